/*
 * oxcull.h -- C ABI of the MI355X-native meshlet visibility pipeline (liboxcull.so).
 *
 * Drop-in boundary for the Oxylus engine's compute-path cull.  The engine has no plugin/FFI
 * table for this path; the boundary is the two RendererInstance members
 *
 *   auto generate_hiz(this RendererInstance&, MainGeometryContext&) -> void;
 *   auto cull_geometry(this RendererInstance&, CullGeometryContext&) -> void;
 *       (Oxylus/include/Render/RendererInstance.hpp:397-398, bodies in
 *        Oxylus/src/Render/Passes/CullGeometry.cpp:10-59 and :61-404)
 *
 * plus their context structs (RendererInstance.hpp:143-216).  This header is the plain-C
 * surface under a C++ shim that keeps those names (oxylus_amd/host/RendererInstance.hpp):
 * every vuk::Value<vuk::Buffer> becomes {device pointer, bytes}, every
 * vuk::Value<vuk::ImageAttachment> becomes a linear mip chain in device memory.  All buffers
 * use the reference's GPU byte layouts (Oxylus/include/Scene/SceneGPU.hpp:84-152,222-229), so a
 * Vulkan consumer could bind the outputs unchanged.
 *
 * Conventions: POD structs only, no exceptions cross the ABI, every entry point returns an
 * oxc_status.  A context is externally synchronised (the reference calls these from the main thread
 * only, RenderContext.cpp:585-586) and owns ONE set of scratch buffers (instance cache, survivor
 * bitmaps, chunk counts), so its calls are ordered: a call on a different hipStream_t than the
 * context's previous call first waits (hipStreamWaitEvent, on the device) for that previous call.
 * (Not across a HIP-graph capture: while hip_stream is being captured that wait is skipped -- work the context still has in flight
 * on another stream must be complete, or ordered by the caller's own events inside the capture, before the capture begins; and a
 * stream the context was last used on must outlive the next call on a different stream, or be synchronised before it is destroyed.)
 * Independent work that should overlap -- a main view and a shadow view, several frames in flight
 * -- uses one context per stream.  All work is enqueued asynchronously on the caller's hipStream_t
 * (passed as void*).  Entry points that synchronise the host: oxc_read_counters (and the test / measurement
 * hooks of oxcull_debug.h: oxc_debug_read_u32, oxc_profile_end), and any call that has to GROW scratch memory (oxc_reserve up front avoids that;
 * while the stream is being captured into a HIP graph a call that would have to grow returns
 * OXC_INVALID_ARG instead).
 */
#ifndef OXCULL_H
#define OXCULL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OXC_ABI_VERSION 5u

typedef struct oxc_ctx oxc_ctx;

typedef enum oxc_status {
  OXC_OK = 0,
  OXC_INVALID_ARG = 1,
  OXC_HIP_ERROR = 2,
  OXC_RCCL_ERROR = 3,
  OXC_OUT_OF_MEMORY = 4
} oxc_status;

/* GPU::CullFlag, SceneGPU.hpp:345-353 (spec constant 0 of every cull pipeline,
 * CullGeometry.cpp:89,156,298,363).  HAS_FLAG(mask, a|b) in the shaders means "any of". */
enum {
  OXC_CULL_NONE = 0u,
  OXC_CULL_TEST_FRUSTUM = 1u << 0,
  OXC_CULL_SELECT_LOD = 1u << 1,
  OXC_CULL_TEST_OCCLUSION = 1u << 2,
  OXC_CULL_LATE_PASS = 1u << 3,
  OXC_CULL_TEST_ALL = 7u
};

/* Which stages of cull_geometry to run (extension; 0 = all, as the reference always does).
 * Used by the benchmark for the "frustum+cone cull only" configuration. */
enum {
  OXC_STAGE_MESHES = 1u << 0,    /* cull_meshes   (only honoured when init_cull_meshes) */
  OXC_STAGE_MESHLETS = 1u << 1,  /* cull_meshlets / cull_meshlets_hiz */
  OXC_STAGE_TRIANGLES = 1u << 2, /* cull_triangles */
  OXC_STAGE_ALL = 7u
};

/* vuk::Value<vuk::Buffer> stand-in: device pointer + size. */
typedef struct oxc_buffer {
  void* dptr;
  uint64_t bytes;
} oxc_buffer;

/* vuk::Value<vuk::ImageAttachment> stand-in for R32F / D32F images: a linear, row-major mip
 * chain in one device allocation.  Level k is max(1,width>>k) x max(1,height>>k) floats at
 * byte offset level_offset[k]. */
typedef struct oxc_image {
  void* dptr;
  uint32_t width, height, levels, _pad;
  uint64_t level_offset[13]; /* bytes; hiz.slang binds at most 13 mips (CullGeometry.cpp:24,36-38) */
} oxc_image;

/* R8UI Texture2DArray with mips (the VSM hierarchical page buffer, `hpb_attachment`): level k
 * holds `layers` planes of max(1,width>>k) x max(1,height>>k) bytes at byte offset level_offset[k]. */
typedef struct oxc_image_array_u8 {
  void* dptr;
  uint32_t width, height, layers, levels;
  uint64_t level_offset[13];
} oxc_image_array_u8;

/* GPU::VirtualClipmap (SceneGPU.hpp:335-339), 76 bytes: the element type of vsm_clipmaps_buffer. */
typedef struct oxc_virtual_clipmap {
  float projection_view_mat[16];
  int32_t page_offset[2];
  float z_near;
} oxc_virtual_clipmap;

/* GPU::CullCamera -- 96 B push constant (SceneGPU.hpp:222-229, scene.slang:196-203). */
typedef struct oxc_cull_camera {
  float projection_view[16]; /* glm::mat4, column-major */
  float position[3];
  float acceptable_lod_error;
  float resolution[2];
  float near_clip;
  uint32_t mesh_instance_count;
} oxc_cull_camera;

/* The PreparedFrame buffers the cull path touches (RendererInstance.hpp:143-169; sizes from
 * RendererInstance.cpp:1640-1732).  Caller-owned device memory. */
typedef struct oxc_prepared_frame {
  uint32_t mesh_instance_count;
  uint32_t max_meshlet_instance_count;
  oxc_buffer meshes_buffer;                           /* GPU::Mesh[]            read  */
  oxc_buffer transforms_world_buffer;                 /* GPU::TransformWorld[]  read  */
  oxc_buffer mesh_instances_buffer;                   /* GPU::MeshInstance[]    read; lod_index written by cull_meshes */
  oxc_buffer meshlet_instances_buffer;                /* GPU::MeshletInstance[] written by cull_meshes, read after */
  oxc_buffer visible_meshlet_instances_indices_buffer; /* u32[max_meshlet_instance_count] written */
  oxc_buffer meshlet_instance_visibility_mask_buffer; /* u32[ceil(N/32)] persistent, read+written when use_hiz */
  oxc_buffer reordered_indices_buffer;                /* u32[N*64*3] written by cull_triangles */
} oxc_prepared_frame;

/* CullGeometryContext (RendererInstance.hpp:171-197).  Field names are the reference's. */
typedef struct oxc_cull_geometry_context {
  uint32_t struct_size; /* sizeof(oxc_cull_geometry_context), for ABI evolution */
  uint32_t use_hiz;     /* cull_meshlets_hiz path (two-pass occlusion) */
  uint32_t use_hpb;     /* cull_meshlets_hpb path (VSM multi-view page cull) */
  uint32_t init_cull_meshes;
  uint32_t cull_flags;  /* OXC_CULL_* */
  uint32_t stages;      /* OXC_STAGE_*; 0 = all */
  oxc_cull_camera cull_camera;
  oxc_image hiz_attachment; /* read when use_hiz */
  /* read when use_hpb (RendererInstance.hpp:183-192, Shadowmaps.cpp:433-463) */
  oxc_image_array_u8 hpb_attachment;
  oxc_buffer vsm_clipmaps_buffer;            /* oxc_virtual_clipmap[vsm_clipmap_count] */
  oxc_buffer vsm_clipmap_dirty_flags_buffer; /* u32[vsm_clipmap_count] */
  uint32_t vsm_clipmap_count;                /* <= 16 */
  /* Extension (no reference behaviour): 0 = the reference's packed index (id << 8) | (3t+k),
   * 64 triangles per meshlet; 1 = wide index (id << 9) | (3t+k) for meshlets of up to 128 triangles
   * (at most 2^23 meshlet instances per call, reordered_indices_buffer >= N*128*3*4 bytes);
   * 2 = SURVEY A.7's form for larger shards: every index is the PAIR {u32 meshlet_instance_index, u32 3t+k}
   * (8 bytes, little endian, id first), meshlets of up to 128 triangles, no id limit below 2^32,
   * reordered_indices_buffer >= N*128*3*8 bytes, same order of entries as the packed forms.  The decode of
   * visbuffer.slang:9-14 becomes instance = pair.x, corner = pair.y (oxc_draw_visbuffer does that).
   * DrawIndexedIndirect.index_count stays the number of INDICES (3 per triangle) and stays a u32: a call that
   * emits more than 2^32 - 1 of them (possible only when N*384 >= 2^32, i.e. N > 11 184 810, and then only if
   * nearly every triangle passes) sets instanceCount = 0 -- the command draws nothing -- and oxc_read_counters
   * of that call returns OXC_INVALID_ARG; every write stays inside the buffer. */
  uint32_t wide_triangle_index;
  /* Extension named by the north star ("per-triangle backface + small-triangle cull"); the reference has only the
   * clip-z and backface tests (cull_triangles.slang:68-69, cull.slang:169-171).  0 (default) = reference behaviour,
   * output byte-identical to a build without the flag.  1 = a triangle that passed both reference tests is ALSO
   * dropped when its screen-space bounding box covers no pixel centre of a cull_camera.resolution target:
   *   per corner (only when all three clip.w > 0, otherwise the triangle is kept):
   *     s.x = ((clip.x / clip.w) * 0.5 + 0.5) * resolution.x,  s.y likewise     (IEEE binary32, no contraction)
   *   lo = min over corners, hi = max over corners (per axis)
   *   dropped iff floor(lo.x + 0.5) == floor(hi.x + 0.5) || floor(lo.y + 0.5) == floor(hi.y + 0.5)
   * (pixel centres sit at k + 0.5: an interval [lo, hi] holds one iff the two roundings differ).  Not supported by
   * the fused path of oxc_cull_geometry_batch (such elements are processed one after the other). */
  uint32_t small_triangle_cull;
  /* EXPERIMENTAL extension (scheduling only, no effect on any output byte; on MI355X it has not been faster than the in-order call in any
   * measured configuration -- both stages keep the vector ALUs and the memory system busy, DESIGN.md 4c -- and exists for engines whose
   * draw sits between the two calls): 1 = the triangle stage of this call (cull_triangles test + ordered
   * emit) is enqueued on a second stream the context owns and runs BESIDE whatever is enqueued on hip_stream next -- typically the
   * meshlet stage of the following oxc_cull_geometry call (ALU-bound, while the triangle stage is HBM-bound) and oxc_generate_hiz.
   * reordered_indices_buffer and draw_geometry_cmd_buffer of this call are complete on a stream only after
   * oxc_join_triangles(ctx, that stream); every oxc_* entry point that reads them (oxc_read_counters, oxc_pack_counters,
   * oxc_draw_visbuffer) joins by itself.  The context orders everything it owns or writes: a later call waits where it would
   * overwrite what a pending triangle stage still reads (the visible list, MeshletInstance records rewritten by cull_meshes, its own
   * scratch).  0 (default) = the whole call is in order on hip_stream, as the reference records it. */
  uint32_t async_triangles;
  /* Extension (caching only, no effect on any output byte): the two HiZ calls of a frame -- early, then OXC_CULL_LATE_PASS, as
   * RendererInstance.cpp:842-884 records them -- run the same frustum and normal-cone tests on the same operands (the camera, the
   * transforms and the MeshletInstance list do not change between them; only the pyramid and the mask do).  With 1 on BOTH calls the
   * early call also evaluates the cone for the meshlets that were not visible last frame and leaves one "passed frustum and cone" bit
   * per meshlet in the context's scratch, and the late call reads those bits instead of testing again (its meshlets outside the
   * frustum are not even fetched).  By setting it on the late call the caller states that nothing those tests read has been written
   * since the early call: meshes / transforms / mesh instances / MeshletInstance list / meshlet bounds.  What the context can
   * check it checks -- the late call reuses the bits only if the previous flagged early call on this context had the same cull_camera
   * (all 96 bytes), the same buffers, counts and flags, and no call in between rebuilt the list (init_cull_meshes) or the scratch;
   * otherwise it silently tests again.  (The match is made when the call is enqueued: a late call captured into a HIP graph on its own
   * reuses, at every replay, the bits of whatever flagged early call ran last -- capture the pair, or keep the scene unchanged
   * between the replays.)  An early call that is in order on one stream (no async_triangles) also does the prepare work of the late call
   * that follows it directly (same capture, if any), which then launches no prepare kernel.  Only with use_hiz
   * and OXC_CULL_TEST_OCCLUSION; ignored elsewhere and by oxc_cull_geometry_batch.  0 (default) = every call tests on its own. */
  uint32_t share_pass_tests;
  /* Extension (output ORDER only; counts and the SET of emitted ids / packed triangles are those of the ordered form, and the mask bytes
   * are identical): how the compacted lists are laid out.  The reference allocates output slots with atomics -- one atomic_add per
   * 64-thread workgroup in cull_meshlets.slang:55-70 and cull_triangles.slang:71-88, two per visible thread in
   * cull_meshlets_hiz.slang:67-78 -- so its order is whatever the race gives.
   *   0 (default) = ascending lists, deterministic: test -> ballots -> ordered emit, two launches per stage.
   *   1 = unordered where that is the faster form on this part: the triangle stage is ONE launch (a block tests a span of visible
   *       meshlets -- implementation-defined, currently 128 -- and appends its packed indices behind one atomic_add on index_count);
   *       the plain meshlet stage (no use_hiz / use_hpb) is one launch (one atomic_add on cull_triangles_cmd.x per 1024 meshlets).
   *       The HiZ / HPB meshlet stages keep the ordered two-launch form and their ascending visible list.
   *   Any other value returns OXC_INVALID_ARG.  (Rounds 4 built "2": the HiZ meshlet tests appending with one atomic_add pair per
   *   256-meshlet wave step, the reference's literal scheme aggregated through the ballot -- 150 / 154 us per launch against 79 + 11 /
   *   66 + 11 for test + ordered emit, every step queueing on two addresses that retire ~88 atomics per microsecond; removed in round 5,
   *   the measurement is in DESIGN.md.)
   * Inside a block's run the ids ascend; the runs land in arrival order.  A triangle's three packed indices stay adjacent.  Sorting a
   * list gives the bytes of the ordered form (tests/test_gpu_unordered.py).  Ignored by oxc_cull_geometry_batch's fused path. */
  uint32_t unordered_output;
  /* Extension (configs[4]: many views of one scene): 1 = cull_meshes leaves this view's MeshletInstance list IMPLICIT instead of writing
   * one 8-byte record per meshlet and view (466 MB per 16 cascade views of a 10 M-meshlet scene, a third of the call): record i of the
   * view is {mesh instance m, meshlet i - first[m]} for first[m] <= i < first[m] + count[m], with {first[m], count[m]} written to
   * meshlet_instance_runs_buffer (u32[2 * mesh_instance_count]; count 0 = the view's cull_meshes dropped the instance) -- "emit runs,
   * expand in the consumer".  visible_meshlet_instances_indices, the counters and lod_index are exactly those of the explicit form;
   * expanding the runs gives the explicit list byte for byte (tests/test_gpu_round2.py).  Only oxc_cull_geometry_batch's multi-view path
   * has no reader of the records (its meshlet test walks the instances' bounds directly), so only there is the flag accepted: every
   * element must set it, stages must not include OXC_STAGE_TRIANGLES; any other call with the flag returns OXC_INVALID_ARG.  The
   * runs buffer alone (flag 0) is also filled by that path when given. */
  uint32_t implicit_meshlet_instances;
  uint32_t _reserved1; /* must be 0 */
  /* in/out: produced when init_cull_meshes, consumed (and updated) by later calls of the
   * sequence, exactly like the reference's hoisted context (RendererInstance.cpp:793-800). */
  oxc_buffer visibility_buffer;        /* GPU::MeshletInstanceVisibility {total, early, late} */
  oxc_buffer cull_meshlets_cmd_buffer; /* VkDispatchIndirectCommand {x, 1, 1} */
  /* out: fresh per call (CullGeometry.cpp:125-127, 380-382) */
  oxc_buffer cull_triangles_cmd_buffer; /* VkDispatchIndirectCommand {#visible meshlets, 1, 1} */
  oxc_buffer draw_geometry_cmd_buffer;  /* VkDrawIndexedIndirectCommand {indexCount, 1, 0, 0, 0} */
  /* out, optional, caller-owned: {first, count} of every mesh instance in this view's MeshletInstance list (see implicit_meshlet_instances) */
  oxc_buffer meshlet_instance_runs_buffer;
} oxc_cull_geometry_context;

/* MainGeometryContext fields used by generate_hiz (RendererInstance.hpp:199-216). */
typedef struct oxc_main_geometry_context {
  uint32_t struct_size;
  uint32_t _pad;
  oxc_image depth_attachment; /* levels = 1; read */
  oxc_image hiz_attachment;   /* written: all `levels` mips */
} oxc_main_geometry_context;

typedef struct oxc_counters {
  uint32_t total_visible_meshlet_instances; /* visibility[0] */
  uint32_t early_visible_meshlet_instances;
  uint32_t late_visible_meshlet_instances;
  uint32_t cull_meshlets_cmd_x;
  uint32_t cull_triangles_cmd_x; /* meshlets emitted by this call */
  uint32_t draw_index_count;     /* 3 * triangles emitted by this call */
} oxc_counters;

/* ---- lifetime ---- */
uint32_t oxc_abi_version(void);
oxc_status oxc_create(int device, oxc_ctx** out);
void oxc_destroy(oxc_ctx* ctx);
const char* oxc_last_error(const oxc_ctx* ctx);

/* Pre-size the context's scratch memory (instance cache, survivor bitmaps, chunk counters) so
 * that no later call allocates.  Optional: calls grow scratch on demand (with a device sync). */
oxc_status oxc_reserve(oxc_ctx* ctx, uint32_t max_mesh_instances, uint32_t max_meshlet_instances);

/* ---- the two reference entry points ---- */
/* Replaces RendererInstance::generate_hiz (Passes/CullGeometry.cpp:10-59, passes/hiz.slang).
 * Limits (else OXC_INVALID_ARG, nothing launched): the pyramid at most 4096 a side with 1..13 levels, every level offset a multiple of 4
 * bytes; either both sides multiples of 64 (then mip 0 16-byte and mip 1 8-byte aligned: they are stored as vectors) or at most 4096 texels.
 * Zeros: the reduction is min with -0.0 < +0.0 (the device's v_min_f32), whatever the order of the operands -- the reference's `min` leaves
 * the sign of a zero result open, this library and its checker pin that one.  A NaN operand is dropped (fminf). */
oxc_status oxc_generate_hiz(oxc_ctx* ctx, const oxc_main_geometry_context* context, void* hip_stream);

/* Replaces RendererInstance::cull_geometry (Passes/CullGeometry.cpp:61-404; kernels
 * passes/cull_meshes.slang, cull_meshlets.slang, cull_meshlets_hiz.slang, cull_triangles.slang).
 * Output lists are written in ascending order (a valid outcome of the reference's
 * atomic-ordered output, and a deterministic one) unless context->unordered_output asks for the
 * reference's own atomic slot allocation. */
oxc_status oxc_cull_geometry(oxc_ctx* ctx, const oxc_prepared_frame* frame, oxc_cull_geometry_context* context,
                             void* hip_stream);

/* Makes `hip_stream` wait (on the device) for every triangle stage this context still has in flight on its own stream
 * (calls made with async_triangles = 1).  Cheap when nothing is pending.  While hip_stream is being captured into a HIP graph the
 * context's stream is part of the capture from the first async call on: join before hipStreamEndCapture. */
oxc_status oxc_join_triangles(oxc_ctx* ctx, void* hip_stream);

/* Batched form: semantically `for i < count: oxc_cull_geometry(ctx, &frames[i], &contexts[i], stream)` for
 * INDEPENDENT frames (no buffer of one element is written by another) -- several views or scenes culled per
 * launch, the way the reference's cull_meshlets_hpb handles all clipmap views in one dispatch.  When every
 * element uses the plain pipeline (use_hiz == use_hpb == 0, no LatePass) with the same `stages` and
 * `init_cull_meshes`, and count <= 16, each stage is ONE launch with grid.y = count; otherwise the elements
 * are processed one after the other.  A 1M-meshlet call is launch-latency bound on MI355X (a HIP graph
 * sustains ~3 us per kernel node); batching is what amortises it.
 * When, in addition, every element runs cull_meshes (init_cull_meshes, OXC_STAGE_MESHES) over the SAME meshes_buffer and
 * transforms_world_buffer with the same flags -- several views of one scene: shadow cascades, BASELINE configs[4] -- the meshlet
 * stage runs once for all views: the views that kept a mesh instance at the same LOD are tested against one load of its
 * MeshletBounds records.  Outputs are the per-element outputs of the plain form, byte for byte. */
oxc_status oxc_cull_geometry_batch(oxc_ctx* ctx, uint32_t count, const oxc_prepared_frame* frames,
                                   oxc_cull_geometry_context* contexts, void* hip_stream);

/* Harness helper: start a cull sequence from a caller-provided MeshletInstance list instead of
 * running cull_meshes (fills context->visibility_buffer = {total,0,0} and
 * cull_meshlets_cmd_buffer = {ceil(total/64),1,1}).  The reference always derives these from
 * cull_meshes; the synthetic benchmark configurations start from a given list.
 * Counter buffers handed back in a context (visibility / cull_meshlets_cmd / cull_triangles_cmd /
 * draw_geometry_cmd) are callee-owned slots of a ring: a seeded pair stays valid for 4096 further seeds, a
 * per-call set for 4096 further cull_geometry / cull_terrain calls (a batched call uses one per element; an early call with
 * share_pass_tests takes the late call's set with its own) on the same oxc_ctx. */
oxc_status oxc_seed_meshlet_instances(oxc_ctx* ctx, oxc_cull_geometry_context* context, uint32_t total,
                                      void* hip_stream);

/* Synchronising readback of the counters a context points at (bench / tests). */
oxc_status oxc_read_counters(oxc_ctx* ctx, const oxc_cull_geometry_context* context, oxc_counters* out,
                             void* hip_stream);

/* ---- meshlet bounds producer (asset side) ---------------------------------------
 * Replaces the per-meshlet loop of Oxylus/src/Asset/AssetManager_GLTF.cpp:683-744 (AABB of the referenced
 * vertices -> meshopt_quantizeHalf, normal cone of meshopt_computeMeshletBounds -> cone_axis_s8 /
 * cone_cutoff_s8, running mesh AABB) and the position quantisation of :573-578.  meshopt_buildMeshlets itself
 * (the greedy clusteriser that produces `meshlets`, `indirect_vertex_indices`, `local_triangle_indices`) stays
 * on the host, as in the reference.  All pointers are device pointers.
 * NaN normals (a cross product that overflowed to inf - inf at coordinates around 1e20, NaN coordinates) count as valid
 * triangles, since `area == 0` is false.  Every compare with a NaN is false, so they are never extremal, never grow the
 * sphere and never lower the minimum dot; a meshlet whose other normals fix the axis gets the cone of those.  Where the NaN
 * reaches the axis (every normal NaN, or the first one with no other to replace it) the minimum dot stays 1, each NaN axis
 * component is stored as cone_axis_s8 = -127 (meshopt_quantizeSnorm clamps before it converts: NaN -> -1), and
 * cone_cutoff_s8 = 0: the sum of the quantisation errors is NaN, and its float -> int conversion gives 0 (v_cvt_i32_f32).
 * NaN coordinates never enter an AABB (`b < a ? b : a` keeps a). */
typedef struct oxc_meshlet_bounds_desc {
  uint32_t struct_size;
  uint32_t vertex_count;
  uint32_t meshlet_count;
  uint32_t _pad;
  oxc_buffer positions;               /* in:  glm::vec3[vertex_count] (float3, stride 12)             */
  oxc_buffer meshlets;                /* in:  GPU::Meshlet[meshlet_count] (SceneGPU.hpp:97-103)       */
  oxc_buffer indirect_vertex_indices; /* in:  u32, indexed by Meshlet::indirect_vertex_index_offset   */
  oxc_buffer local_triangle_indices;  /* in:  u8,  indexed by Meshlet::local_triangle_index_offset    */
  oxc_buffer meshlet_bounds;          /* out: GPU::MeshletBounds[meshlet_count] (SceneGPU.hpp:84-90)  */
  oxc_buffer mesh_bounds;             /* out: GPU::MeshBounds {vec3 aabb_center; vec3 aabb_extent} (SceneGPU.hpp:92-95) */
  oxc_buffer quantized_positions;     /* out, optional (dptr may be NULL): u16x4[vertex_count]        */
} oxc_meshlet_bounds_desc;

oxc_status oxc_build_meshlet_bounds(oxc_ctx* ctx, const oxc_meshlet_bounds_desc* desc, void* hip_stream);

/* ---- SURVEY 8(f)-1, format side: vertex streams and the mesh blob ---------------------------------
 * oxc_quantize_vertex_streams replaces the three per-vertex loops of AssetManager_GLTF.cpp:570-588:
 *   positions -> u16x4 {half(x), half(y), half(z), 0}                     (:571-575, meshopt_quantizeHalf)
 *   normals   -> u32 ((snorm10(x)+511) << 20) | ((snorm10(y)+511) << 10) | (snorm10(z)+511)
 *                                                                         (:578-582, meshopt_quantizeSnorm(v, 10))
 *   texcoords -> u16x2 {half(u), half(v)}                                 (:585-588)
 * A stream whose input dptr is NULL is skipped (its output is not touched).  Device pointers. */
typedef struct oxc_vertex_streams_desc {
  uint32_t struct_size;
  uint32_t vertex_count;
  oxc_buffer positions;           /* in, optional:  glm::vec3[vertex_count] */
  oxc_buffer normals;             /* in, optional:  glm::vec3[vertex_count] */
  oxc_buffer texcoords;           /* in, optional:  glm::vec2[vertex_count] */
  oxc_buffer quantized_positions; /* out: u16x4[vertex_count] */
  oxc_buffer quantized_normals;   /* out: u32[vertex_count]   */
  oxc_buffer quantized_texcoords; /* out: u16x2[vertex_count] */
} oxc_vertex_streams_desc;

oxc_status oxc_quantize_vertex_streams(oxc_ctx* ctx, const oxc_vertex_streams_desc* desc, void* hip_stream);

/* The mesh blob: one allocation per mesh holding the vertex streams, every LOD's five arrays and, last, the
 * GPU::MeshLOD table (AssetManager_GLTF.cpp:466-474 blob_append, :590-597, :748-752, :768-769).  Offsets follow
 * blob_append's rule offset = align_up(current size, alignment): positions 8, normals 4, texcoords 4 (only when
 * present), then per LOD indices 8, meshlets 8, meshlet_bounds 8, local_triangle_indices 8,
 * indirect_vertex_indices 4, then the LOD table at align_up(size, 8).  Host-only arithmetic: no context, no GPU. */
#define OXC_MESH_MAX_LODS 8u /* GPU::Mesh::MAX_LODS, SceneGPU.hpp:143 */

typedef struct oxc_mesh_lod_counts { /* the *_count fields of GPU::MeshLOD (SceneGPU.hpp:125-139) + error */
  uint32_t indices_count;                 /* u32 elements */
  uint32_t meshlet_count;                 /* GPU::Meshlet (16 B) and GPU::MeshletBounds (16 B) records */
  uint32_t local_triangle_indices_count;  /* u8 elements (last meshlet's run padded to 4, :699) */
  uint32_t indirect_vertex_indices_count; /* u32 elements */
  float error;
} oxc_mesh_lod_counts;

typedef struct oxc_mesh_blob_desc {
  uint32_t struct_size;
  uint32_t vertex_count;
  uint32_t has_texture_coords;
  uint32_t lod_count; /* 1..OXC_MESH_MAX_LODS */
  oxc_mesh_lod_counts lods[OXC_MESH_MAX_LODS];
} oxc_mesh_blob_desc;

typedef struct oxc_mesh_lod_offsets {
  uint64_t indices, meshlets, meshlet_bounds, local_triangle_indices, indirect_vertex_indices;
} oxc_mesh_lod_offsets;

typedef struct oxc_mesh_blob_layout { /* byte offsets from the start of the blob */
  uint64_t size;                /* whole blob, LOD table included */
  uint64_t lod_metadata_offset; /* GPU::MeshLOD[lod_count] */
  uint64_t vertex_positions, vertex_normals, texture_coords; /* texture_coords = 0 when absent */
  oxc_mesh_lod_offsets lods[OXC_MESH_MAX_LODS];
} oxc_mesh_blob_layout;

oxc_status oxc_mesh_blob_layout_of(const oxc_mesh_blob_desc* desc, oxc_mesh_blob_layout* out_layout);

/* upload_gltf_mesh's relocation (AssetManager_GLTF.cpp:780-800): with the blob resident at `device_address`,
 * write the GPU::MeshLOD table (absolute addresses + counts + error) into the HOST copy `blob` at
 * lod_metadata_offset and fill `out_gpu_mesh` (64 B GPU::Mesh: absolute stream addresses, texture_coords 0 when
 * absent, vertex_count, lod_count, lods, bounds = mesh_bounds {aabb_center.xyz, aabb_extent.xyz}).  The caller
 * then copies the blob to the device (the reference's staging upload, :802-818). */
oxc_status oxc_mesh_blob_finalize(const oxc_mesh_blob_desc* desc, const oxc_mesh_blob_layout* layout, uint64_t device_address,
                                  void* blob, uint64_t blob_bytes, const float mesh_bounds[6], void* out_gpu_mesh);

/* ---- SURVEY 8(f)-1, clusteriser side: triangle soup -> LOD chain -> meshlets (host code, as in the reference) ----------
 * Replaces the per-LOD loop of AssetManager_GLTF.cpp:599-682: LOD 0 = the input indices, LOD i = LOD i-1 simplified to half its
 * index count with the border locked (meshopt_simplifyWithAttributes, normal weights 1), error accumulated down the chain, chain
 * cut by the reference's three stop rules (:639-645) or at GPU::Mesh::MAX_LODS; every LOD clustered into meshlets of at most
 * max_vertices / max_triangles (64 / 64: Model::MAX_MESHLET_INDICES / _PRIMITIVES, meshopt_buildMeshlets with cone_weight 0), u8
 * micro-index runs 4-byte aligned (:687).  meshoptimizer is a third-party dependency that is not part of the reference tree: its two
 * algorithms are restated in shape, not heuristic for heuristic (oxylus_amd/csrc/oxcull_meshbuild.cpp) -- a valid, different clustering.
 * LOD 0's `indices` are the input verbatim; triangles with a repeated corner are left out of the meshlets and of the simplifier's input
 * (no area).  `error` accumulates this simplifier's own relative error measure: it orders a mesh's LODs like meshopt's result_error
 * does but is not numerically comparable to it, so CULL_SELECT_LOD thresholds tuned against meshoptimizer do not carry over.
 * Host pointers in, host views out (owned by the handle); feed them to oxc_build_meshlet_bounds / oxc_quantize_vertex_streams /
 * oxc_mesh_blob_* to obtain what oxc_cull_geometry consumes. */
typedef struct oxc_mesh_build oxc_mesh_build;
typedef struct oxc_mesh_build_desc {
  uint32_t struct_size;
  uint32_t vertex_count;
  uint32_t index_count;   /* multiple of 3 */
  uint32_t max_lods;      /* 0 = OXC_MESH_MAX_LODS */
  uint32_t max_vertices;  /* per meshlet, 0 = 64 */
  uint32_t max_triangles; /* per meshlet, 0 = 64 */
  const float* positions; /* glm::vec3[vertex_count] */
  const float* normals;   /* glm::vec3[vertex_count], optional (NULL: positions only) */
  const uint32_t* indices;
} oxc_mesh_build_desc;
/* (LOD 0 of a mesh whose input has degenerate triangles: `indices` / `indices_count` keep them -- the reference passes the index buffer
 * through unchanged -- while the meshlets are built from the non-degenerate ones, so indices_count / 3 can exceed the sum of the meshlets'
 * triangle_count.  Nothing on the cull path reads `indices`; a consumer that draws from them gets the degenerate triangles back, which
 * rasterise nothing.) */
typedef struct oxc_mesh_lod_view { /* the arrays of one GPU::MeshLOD (SceneGPU.hpp:125-139), host memory */
  const uint32_t* indices;
  const void* meshlets; /* GPU::Meshlet[meshlet_count], 16 B each */
  const uint32_t* indirect_vertex_indices;
  const uint8_t* local_triangle_indices;
  uint32_t indices_count, meshlet_count, indirect_vertex_indices_count, local_triangle_indices_count;
  float error;
  uint32_t _pad;
} oxc_mesh_lod_view;
oxc_status oxc_mesh_build_create(const oxc_mesh_build_desc* desc, oxc_mesh_build** out);
uint32_t oxc_mesh_build_lod_count(const oxc_mesh_build* build);
oxc_status oxc_mesh_build_lod(const oxc_mesh_build* build, uint32_t lod, oxc_mesh_lod_view* out);
void oxc_mesh_build_destroy(oxc_mesh_build* build);
/* Replaces meshopt_optimizeVertexFetchRemap as AssetManager_GLTF.cpp:512-568 uses it (host code there too): remap_out[old vertex id] = its
 * rank by first appearance in `stream` (count entries, each < vertex_count); vertices the stream never names follow the used ones in their
 * old order (the reference drops them: *used_out tells how many are used).  The reference passes the raw index buffer, before it simplifies
 * and clusters.  Passing LOD 0's indirect_vertex_indices instead orders the vertices by MESHLET: the <= 64 vertices of a meshlet then lie
 * next to each other in vertex_positions and cull_triangles' position gather touches a handful of cache lines (measured: DESIGN.md 5).  The
 * caller applies the remap to its vertex streams and to every LOD's indices / indirect_vertex_indices; geometry and meshlets do not change. */
oxc_status oxc_mesh_vertex_fetch_remap(const uint32_t* stream, uint64_t count, uint32_t vertex_count, uint32_t* remap_out, uint32_t* used_out);

/* ---- hierarchical page buffer producer ------------------------------------------
 * Replaces the "vsm downsample hpb" pass (Oxylus/src/Render/Passes/Shadowmaps.cpp:331-366, pipeline
 * rmvsm_downsample_hpb, Shaders/passes/rmvsm_downsample_hpb.slang:10-33): level 0 of the pyramid is 1 where
 * the virtual page is Visible && Backed && Dirty (VSMPageState flags 1, 4, 2: rmvsm.slang:16-28,49-70), level i
 * is the OR of the 2x2 children in level i-1 (texels outside the source level read as 0).
 * `virtual_page_table` is the R32UI Texture2DArray as a linear u32 array [layers][height][width];
 * the extent of level i is max(1, width >> i) x max(1, height >> i) (Shadowmaps.cpp:342-346). */
oxc_status oxc_generate_hpb(oxc_ctx* ctx, oxc_buffer virtual_page_table, const oxc_image_array_u8* hpb_attachment, void* hip_stream);

/* ---- VSM page update: mark, allocate and invalidate shadow pages ------------------------------------
 * Replaces the page-management part of RendererInstance::draw_virtual_shadowmap (Oxylus/src/Render/Passes/Shadowmaps.cpp:143-421),
 * the passes the reference runs between the main view's depth buffer and the shadow cull, in its order:
 *   1. sun_moved: the page table is cleared to 0 (:143-148);
 *   2. reset page visibility: Visible, Dirty and Invalidated cleared (passes/rmvsm_reset_page_visibility.slang);
 *   3. invalidate pages, only when !sun_moved && dirty_mesh_instance_count > 0 (:203; rmvsm_invalidate_pages.slang): for each dirty
 *      mesh instance and each clipmap, project_aabb of the mesh AABB through projection_view_mat * previous_world and through
 *      projection_view_mat * world (the cull path's project_aabb, `center - extent * 0.5` corner); every page of the clamped page
 *      rectangle whose entry is Backed becomes exactly Invalidated (8): reset() then set_invalidated, the address bits go too;
 *   4. mark visible pages (rmvsm_mark_visible_pages.slang), one thread per depth pixel, rules below;
 *   5. free invisible pages: an entry that is Backed but not Visible loses the Backed bit only (its address bits stay);
 *   6. build the free page list: physical pages that no Visible && Backed entry names, ascending;
 *   7. allocate pages: request i (Visible, not Backed) gets free_list[i] -- address, Dirty and Backed set -- when
 *      i < free_page_count; otherwise the allocation fails and NOTHING is stored (rmvsm_allocate_pages.slang:35-38 returns before
 *      the Store): the page stays Visible and unbacked, its AllocationFailed bit stays 0, and the failure is counted in
 *      counters_buffer[4] only;
 *   8. HPB downsample when hpb_attachment.dptr != NULL: the bytes of oxc_generate_hpb on the final table;
 *   9. mark dirty pages: every Backed && Dirty entry -- in this sequence, the pages allocated by this call -- appends its physical
 *      page coords (addr % P, addr / P), P = physical_page_table_size / page_size, to dirty_physical_pages_buffer, counts in
 *      clear_cmd.z and sets its layer's dirty flag;
 *  10. clear dirty pages when physical_page_image.dptr != NULL: every texel of every dirty physical page is set to 1.0.
 * Deterministic orders (the reference orders these lists by atomics; each order below is one its race can produce, and the flags and
 * the set of backed pages do not depend on it while no allocation fails): requests are taken in ascending (layer, y, x) order of the
 * wrapped page; the free list is ascending physical index; the dirty list is ascending (layer, y, x).
 * Mark visible pages (binary32, no contraction, IEEE division and square root, the Slang's evaluation order):
 *   a pixel with depth == 0.0 marks nothing;  uv = (float2(x, y) + 0.5) / depth_extent;
 *   unproject(uv, d) = (M (uv * 2 - 1, d, 1)).xyz / w, M = inv_projection_view, each row ((m0 a + m1 b) + m2 c) + m3;
 *   o = (1.0 / resolution) * 0.5, left = uv + (-o.x, o.y), right = uv + (o.x, o.y);
 *   dist = sqrt((dx dx + dy dy) + dz dz) of unproject(left, d) - unproject(right, d);
 *   texel_len = ((first_clipmap_width * (float(n - 1) / float(n))) * 2.0) / virtual_extent, n = page_table_size;  r = dist / texel_len;
 *   clipmap index (the reference's min(u32(ceil(bias + max(log2(r), 0))), count - 1), stated without log2): the number of k in
 *     [0, count - 2] for which (double)k - (double)bias < 0 or (double)r > exp2((double)k - (double)bias) -- a negative ceil gives 0, a
 *     NaN r acts as log2 = 0;
 *   clip = pv (world, 1) of that clipmap, uv' = (clip.xy / clip.w + 1.0) * 0.5; outside [0, 1] (or NaN) marks nothing;
 *   virt = int(floor(uv' * float(n))); virt outside [0, n - 1] marks nothing; wrapped = floor_mod(virt + page_offset, n) (integer,
 *   the result in [0, n)); the entry (clipmap, wrapped.y, wrapped.x) becomes Visible.
 * Limits (else OXC_INVALID_ARG): 1 <= clipmap_count <= 16, page_table_size a multiple of 8 in [8, 256], page_size a multiple of 16,
 * physical_page_table_size a multiple of page_size with at most 65536 physical pages (16 address bits), depth_extent equal to the depth
 * attachment's extent.  The documented configuration is the reference's (RendererInstance.hpp:262-267): page_size 128,
 * page_table_size 64, physical_page_table_size 8192, 10 clipmaps.
 * No host synchronisation; the only allocation is the context's own scratch (the per-page mark map, the free page list), which grows
 * on the first call of a larger shape (not while the stream is captured: OXC_INVALID_ARG then).  Capturable into a HIP graph. */
typedef struct oxc_vsm_update_context {
  uint32_t struct_size; /* sizeof(oxc_vsm_update_context) */
  uint32_t sun_moved;   /* RMVSMContext::sun_moved */
  /* the GPU::VSMContext fields the passes read (rmvsm.slang:116-127, SceneGPU.hpp:325-337) */
  int32_t page_size;                /* texels per page side */
  int32_t page_table_size;          /* n: virtual pages per table side */
  int32_t physical_page_table_size; /* VSMContext::physcial_page_table_size: physical image side in texels */
  int32_t clipmap_count;            /* layers of the page table */
  int32_t depth_extent[2];
  float first_clipmap_width;
  float clipmap_selection_bias;
  float virtual_extent;
  uint32_t dirty_mesh_instance_count; /* PreparedFrame::dirty_mesh_instance_count */
  /* the GPU::Camera fields the passes read (scene.slang:162-193) */
  float inv_projection_view[16]; /* column-major */
  float resolution[2];
  oxc_buffer virtual_page_table;  /* in/out, persistent across frames: u32 [clipmap_count][n][n] VSMPageMetadata (rmvsm.slang:16-112) */
  oxc_buffer vsm_clipmaps_buffer; /* in: oxc_virtual_clipmap[clipmap_count] */
  oxc_image depth_attachment;     /* in: R32F, levels = 1, the main view's reversed-Z depth (0 = nothing drawn) */
  oxc_buffer dirty_mesh_instance_indices; /* in (pass 3): u32[dirty_mesh_instance_count] */
  oxc_buffer mesh_instances_buffer;       /* in (pass 3): GPU::MeshInstance[] */
  oxc_buffer meshes_buffer;               /* in (pass 3): GPU::Mesh[] */
  oxc_buffer transforms_world_buffer;     /* in (pass 3): GPU::TransformWorld[] */
  oxc_buffer transforms_previous_buffer;  /* in (pass 3): GPU::TransformPrevious[] (one mat4, SceneGPU.hpp:24-26) */
  oxc_buffer vsm_clipmap_dirty_flags_buffer; /* out: u32[clipmap_count], every layer written 0 or 1 (what oxc_cull_geometry(use_hpb) reads) */
  oxc_buffer dirty_physical_pages_buffer;    /* out: u32x2 dirty_physical_page_coords, one per dirty page (room for min(pages, P * P)) */
  oxc_buffer clear_cmd_buffer;               /* out: VkDispatchIndirectCommand {page_size / 16, page_size / 16, dirty count}, z counted from 0 */
  oxc_buffer counters_buffer;                /* out: u32[8] {active_request_count, dirty_physical_page_count, free_page_count, alloc_cursor,
                                                failed allocations, 0, 0, 0} (VSMPageAllocator's four counts, then the failures) */
  oxc_image_array_u8 hpb_attachment;         /* optional out (dptr NULL: skipped): width = height = n, layers = clipmap_count */
  oxc_image physical_page_image;             /* optional out (dptr NULL: skipped): R32F, levels = 1, physical_page_table_size square */
} oxc_vsm_update_context;

oxc_status oxc_update_virtual_shadowmap(oxc_ctx* ctx, const oxc_vsm_update_context* context, void* hip_stream);

/* ---- VSM shadow draw: rasterise the shadow cull's triangles into the dirty physical pages ----------------
 * Replaces the tail of RendererInstance::draw_virtual_shadowmap (Shadowmaps.cpp:466-754): rmvsm_build_draw_commands, then the
 * indirect multi-draw of rmvsm_draw_physical_pages (vs_main / fs_main), as a compute rasteriser.  The frame is
 *   oxc_update_virtual_shadowmap -> oxc_cull_geometry(use_hpb, the last clipmap's camera, Shadowmaps.cpp:433-463) -> this call,
 * with `frame` and draw_geometry_cmd_buffer / wide_triangle_index of that cull.
 *   active clipmaps  (rmvsm_build_draw_commands) those whose dirty flag is not 0, in DESCENDING clipmap index.  When the three optional
 *           buffers are given, active clipmap number i gets draw_commands[i] = a copy of the 5 words of the source command,
 *           draw_clipmaps[i] = its index, and draw_count = the number of active clipmaps (entries past it are not written).  All of it
 *           is worked out on the device; nothing is read back to the host.
 *   vertex  each index of the list is drawn once per active clipmap.  Vertex fetch, world, the clipper (w >= 2^-10 and the 64x guard
 *           band), the screen mapping, the 1/256-pixel snap, the top-left rule and the binary64 z/w interpolation from exact edge values
 *           are exactly oxc_draw_visbuffer's, with projection_view = that clipmap's projection_view_mat and a V x V viewport,
 *           V = page_table_size * page_size.  A command with instanceCount == 0 draws nothing (the pair form's overflow rule); any other
 *           instanceCount draws the list once.  indexCount / 3 triangles are drawn (a remainder of 1 or 2 indices is ignored), at most
 *           those the index buffer holds.  firstIndex, vertexOffset and firstInstance (words 2..4) are copied to draw_commands verbatim
 *           and have no other effect: the list is read from its start.
 *   cull    None (Shadowmaps.cpp: cullMode eNone): a triangle with negative fixed-point area is re-oriented (corners 1 and 2 swapped),
 *           one with positive area is kept as is, zero area covers nothing; the top-left rule applies after orientation, so a shared
 *           edge is covered exactly once whatever the windings.
 *   depth   z = the interpolated value rounded to binary32; a fragment is kept when 0.0 <= z && z <= 1.0 (NaN is dropped).  For the
 *           clipmaps' orthographic matrices (w = 1) this is the reference's position.z / position.w; there are no z clip planes, the
 *           test stands in for them.
 *   page    (fs_main, in integers) for pixel (x, y) of clipmap c: virtual page v = (x / page_size, y / page_size), wrapped =
 *           floor_mod(v + page_offset, n), e = virtual_page_table[c][wrapped.y][wrapped.x].  The fragment writes only when e is
 *           Backed && Dirty and its address addr = e >> 16 names a physical page (addr < P * P, P = physical_page_table_size /
 *           page_size; an out-of-range image store does nothing in Vulkan either); its texel is (addr % P, addr / P) * page_size +
 *           (x % page_size, y % page_size).  When physical_page_table_size == V and the sizes are powers of two this equals the
 *           reference's float form (virtual_uv = position.xy / physical extent; the reference's shape is 8192 = 64 x 128).
 *   write   atomicMin on the texel's u32 bits (the reference's __atomic_min(asuint(z))): a -0.0 fragment never lowers a stored value.
 *           The result does not depend on the order of the fragments: the image is deterministic byte for byte.
 *   materials are not read: every material is drawn opaque.  (Stated difference: the reference's alpha-cutoff test samples albedo
 *           textures, and this library has no textures.)
 * Limits (else OXC_INVALID_ARG): the shape limits of oxc_update_virtual_shadowmap, V <= 16384 (the guard band's fixed-point range),
 * physical_page_image one 16-byte aligned R32F level of exactly physical_page_table_size^2, wide_triangle_index 0..2, the optional
 * outputs all given or all absent.  The context's scratch (drawable-page bitmaps, per-instance rows, the big-triangle / tile / clip
 * queues, one entry per (triangle, clipmap) pair the index buffer can hold, 4096..2^24) grows on the first call of a larger shape or
 * frame, with a device synchronisation (not while the stream is captured: a call that would need larger bitmaps or rows returns
 * OXC_INVALID_ARG then, one that would only want larger queues uses the current ones).  Past a queue, overflow passes find the pairs
 * again and draw them with whole waves: slower, the same image.  No host synchronisation otherwise; capturable into a HIP graph.
 * Work: a prologue launch reads the page table once and builds, per active clipmap, a bitmap of drawable virtual pages and their
 * bounding rectangle; the triangle pass drops every (triangle, clipmap) pair whose page box holds no drawable page, and a large
 * triangle is rasterised per drawable page of its page box only -- with no active clipmap the call costs its launches only. */
typedef struct oxc_vsm_draw_context {
  uint32_t struct_size;         /* sizeof(oxc_vsm_draw_context) */
  uint32_t wide_triangle_index; /* 0 / 1 / 2, same meaning as in oxc_cull_geometry_context */
  int32_t page_size, page_table_size, physical_page_table_size, clipmap_count; /* as in oxc_vsm_update_context */
  oxc_buffer draw_geometry_cmd_buffer;       /* in: the shadow cull's VkDrawIndexedIndirectCommand, read on the device */
  oxc_buffer virtual_page_table;             /* in: u32 [clipmap_count][n][n] */
  oxc_buffer vsm_clipmaps_buffer;            /* in: oxc_virtual_clipmap[clipmap_count] (projection_view_mat, page_offset) */
  oxc_buffer vsm_clipmap_dirty_flags_buffer; /* in: u32[clipmap_count] */
  oxc_image physical_page_image;             /* in/out: R32F, one level, physical_page_table_size square */
  oxc_buffer draw_commands_buffer;           /* optional out: VkDrawIndexedIndirectCommand[clipmap_count] */
  oxc_buffer draw_count_buffer;              /* optional out: u32 */
  oxc_buffer draw_clipmaps_buffer;           /* optional out: u32[clipmap_count] */
} oxc_vsm_draw_context;

oxc_status oxc_draw_physical_pages(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_vsm_draw_context* context, void* hip_stream);

/* ---- VSM shadow resolve: the PCSS light-visibility term from the physical pages ----------------------------------
 * Replaces RendererInstance::resolve_shadowmap (Oxylus/src/Render/Passes/Shadowmaps.cpp:756-822, pipeline resolve_shadowmaps,
 * passes/resolve_shadowmaps.slang), the consumer of oxc_update_virtual_shadowmap -> oxc_cull_geometry(use_hpb) -> oxc_draw_physical_pages:
 * one thread per pixel of the main view, one R32F value per pixel, every pixel written.  The reference draws a full-screen triangle to get
 * that thread; nothing else of the graphics pipeline is used.
 * Arithmetic: binary32, no contraction, IEEE division and square root, the Slang's evaluation order; mul(M, v), dot, length and normalize
 * as SURVEY.md A.0 / DESIGN.md section 2 define them; cross(a, b).x = a.y * b.z - a.z * b.y and its rotations (y: a.z * b.x - a.x * b.z,
 * z: a.x * b.y - a.y * b.x), each product rounded before the subtraction; max(a, b) / min(a, b) are fmaxf / fminf (a NaN operand gives the
 * other one); lerp(a, b, t) = a + (b - a) * t; fract(x) = x - floor(x).  The reference is compiled fast-math and is not bit-defined: this is
 * the one evaluation the device and the checker (tests/vsm_resolve_model.py) both follow.
 *   1. sky     depth == 0.0 gives 1.0 (a NaN depth is not sky).
 *   2. set-up  uv = (float2(x, y) + 0.5) / extent of the depth image;  world = unproject(uv, depth) and base = the clipmap index, both
 *              exactly as in oxc_update_virtual_shadowmap's mark pass (same footprint o = (1.0 / resolution) * 0.5, texel_len, thresholds);
 *              e = (.b, .a) of the normal texel, binary16 -> binary32 (exact, denormals kept);  oct_to_vec3(e): v = (e.x, e.y,
 *              (1.0 - |e.x|) - |e.y|), s = (e.x >= 0 ? 1 : -1, e.y >= 0 ? 1 : -1) (a NaN gives -1), when v.z < 0: v.xy = ((1.0 - |e.y|) * s.x,
 *              (1.0 - |e.x|) * s.y); normalize(v);  flat_N = normalize(oct_to_vec3(e)) (two normalisations, as the Slang).
 *   3. pcss    L = directional_light_dir;  NoL = max(dot(N, L), 0.0);  cts = exp2(base + 1) * texel_len (an exact power of two times
 *              texel_len);  b = (1.41421356f * cts) * 0.5;  base_bias = (2^-22 + b) + (NoL < 0.99f ? (b * length(cross(N, L))) / max(NoL, 0.1f)
 *              : b);  inv_z = 1.0 / z_length;  P = world + N * (cts * (1.0 + 2.0 * (1.0 - NoL)));  tangent basis of L alone (computed once
 *              per call): axis = |L.y| < 0.999f ? (0, 1, 0) : (1, 0, 0), T = normalize(cross(axis, L)), B = cross(L, T);
 *              d_recv = (M_base (P, 1)).z / .w, d_recv_world = d_recv * z_length;  centre = tap(P).
 *              Blocker search, i = 0..15: xi = fract(hammersley2d(i, 16) + noise);  r = sqrt(xi.x) * 0.1f;  (c, s) = rotation(xi.y);
 *              offset = r * (T * c + B * s);  bias = inv_z * (base_bias + lerp(2.0 * r, 0.0, NoL));  d = tap(P + offset);  a miss is skipped;
 *              else valid += 1 and, when d + bias < d_recv, accum += d * z_length and blockers += 1.
 *              hard = centre missed ? 1.0 : (centre + inv_z * base_bias < d_recv ? 0.0 : 1.0).
 *              valid == 0 returns hard; blockers == 0 returns 1.0; blockers == valid returns 0.0.
 *              pcf_radius = min(0.1f, (d_recv_world - accum / f32(blockers)) * 0.002f).
 *              PCF, i = 0..23: the same with hammersley2d(i, 24) + noise.yx and r = sqrt(xi.x) * pcf_radius;  a hit adds 1 to
 *              valid_pcf and, when d + bias >= d_recv, 1.0 to light_visibility.
 *   4. tap     (sample_vsm_shadow_depth_with_fallback) the clipmaps base, base - 1, base + 1 in that order; the first that does not miss
 *              gives the depth.  For clipmap c: an index outside [0, clipmap_count) is a miss;  h = M_c (p, 1), clip_uv = (h.xy / h.w + 1.0)
 *              * 0.5 (get_clipmap_info, rmvsm.slang:214-221); a clip_uv outside [0, 1], or NaN, is a miss;  page = int(floor(clip_uv *
 *              float(n))), a page outside [0, n - 1] is a miss;  wrapped = floor_mod(page + page_offset, n);  an entry that is not Backed is
 *              a miss (Visible and Dirty are not consulted), so is one whose address addr = e >> 16 is >= P * P (P = physical_page_table_size /
 *              page_size): it names no physical page and is never loaded;  in-page texel = int(floor(clip_uv * float(V))) % page_size,
 *              V = page_table_size * page_size;  the value is physical_page_image at (addr % P, addr / P) * page_size + in-page texel;  a
 *              stored value equal to -1.0 (the Slang's VSM_DEPTH_MISS) is a miss as well.
 *              Stated difference: the reference multiplies clip_uv by the PHYSICAL extent for the in-page texel; its two extents are both
 *              8192.  V is the viewport oxc_draw_physical_pages rasterises with, so a tap reads the texel the draw wrote for every shape.
 *   5. noise   Stated difference: the reference's hash2 is fract(sin(dot(p, k)) * 43758.5453) on arguments near 10^6, which under fast-math
 *              is not reproducible between two devices.  Here h = pcg2d(x, y) on the u32 pixel coordinate, all operations modulo 2^32:
 *              v = v * 1664525 + 1013904223 (both components); v.x += v.y * 1664525; v.y += v.x * 1664525; v ^= v >> 16 (both); v.x += v.y *
 *              1664525; v.y += v.x * 1664525; v ^= v >> 16 (both);  noise = (f32(h.x >> 8), f32(h.y >> 8)) * 2^-24, in [0, 1).
 *              hammersley2d(i, N) = (f32(i) / f32(N), f32(reversebits(i)) * 2^-32).
 *   6. rotation  Stated difference: (cos, sin) of xi.y * TAU cannot be matched through a library sin.  For t = xi.y (a binary32 in [0, 1)):
 *              q = 4 t (exact), k = floor(q), f = q - k (exact);  f > 0.5: g = 1.0 - f (exact) and the pair below is swapped, else g = f;
 *              in binary64, no contraction: a = (double)g * 0x1.921fb54442d18p+0, z = a * a,
 *                sin = a + (a * z) * (((0x1.71de3a556c734p-19 * z + -0x1.a01a01a01a01ap-13) * z + 0x1.1111111111111p-7) * z + -0x1.5555555555555p-3),
 *                cos = 1.0 + z * ((((-0x1.27e4fb7789f5cp-22 * z + 0x1.a01a01a01a01ap-16) * z + -0x1.6c16c16c16c17p-10) * z + 0x1.5555555555555p-5) * z
 *                      + -0x1.0000000000000p-1),
 *              each rounded to binary32 once (S, C; swapped when f > 0.5);  (c, s) = (C, S), (-S, C), (-C, -S), (S, -C) for k = 0..3.
 *              Each component is within 2^-23 of the exact value (tests/test_vsm_resolve_model.py).
 *   7. result  0.0, 1.0, hard, or light_visibility / f32(valid_pcf) (valid_pcf == 0 returns hard).
 * Limits (else OXC_INVALID_ARG): the shape limits of oxc_update_virtual_shadowmap; depth_attachment and resolved_shadows_attachment one
 * R32F level each, of the same extent (at most 65536 a side); normal_attachment 8-byte aligned with one u16x4 per pixel; physical_page_image
 * one R32F level of exactly physical_page_table_size^2.  One launch, no scratch, no allocation, no host synchronisation; capturable into a
 * HIP graph. */
typedef struct oxc_shadow_resolve_context {
  uint32_t struct_size; /* sizeof(oxc_shadow_resolve_context) */
  /* the GPU::VSMContext fields the pass reads (rmvsm.slang:116-127) */
  int32_t page_size, page_table_size, physical_page_table_size, clipmap_count; /* as in oxc_vsm_update_context */
  float first_clipmap_width;
  float clipmap_selection_bias;
  float virtual_extent;
  float z_length;                 /* the reference sets max_shadow_dist * 2 */
  float directional_light_dir[3];
  /* the GPU::Camera fields the pass reads */
  float inv_projection_view[16];  /* column-major */
  float resolution[2];
  oxc_image depth_attachment;     /* in: R32F, levels = 1, reversed Z, 0 = nothing drawn */
  oxc_buffer normal_attachment;   /* in: the R16G16B16A16Sfloat normal image (RendererInstance.cpp:709-716) as linear u16x4[height][width];
                                     only .b and .a are read: the octahedral world normal visbuffer_decode writes */
  oxc_buffer vsm_clipmaps_buffer; /* in: oxc_virtual_clipmap[clipmap_count] */
  oxc_buffer virtual_page_table;  /* in: u32 [clipmap_count][n][n] */
  oxc_image physical_page_image;  /* in: R32F, levels = 1, physical_page_table_size square */
  oxc_image resolved_shadows_attachment; /* out: R32F, levels = 1, the extent of the depth image */
} oxc_shadow_resolve_context;

oxc_status oxc_resolve_shadowmap(oxc_ctx* ctx, const oxc_shadow_resolve_context* context, void* hip_stream);

/* ---- Contact shadows: the screen-space ray-marched sun shadow term ------------------------------------------------
 * Replaces the contact_shadows pass that follows resolve_shadowmap in RendererInstance::render (Oxylus/src/Render/RendererInstance.cpp:
 * 990-1020, pipeline contact_shadows, passes/contact_shadows.slang + the depth ray marcher raymarch.slang): per pixel of the main view a
 * short ray towards the sun is marched through the depth image; one R32F value per pixel, every pixel written.  pbr_apply.slang:85-87
 * multiplies it with oxc_resolve_shadowmap's value (that product is the consumer's).  Engine defaults (RendererCVar.cpp:30-34): steps 8,
 * thickness 0.1, shadow_length 0.01.
 * Arithmetic: as oxc_resolve_shadowmap (binary32, round to nearest even, no contraction, IEEE division and square root, the Slang's
 * evaluation order; mul(M, v) row by row, left to right; max / min are fmaxf / fminf: a NaN operand gives the other one; lerp(a, b, t) =
 * a + (b - a) * t; 2-component length(v) = sqrt(v.x * v.x + v.y * v.y)).  The reference is compiled fast-math and samples through
 * hardware filtering, so it is not bit-defined: this is the one evaluation the device and the checker (tests/contact_shadows_model.py)
 * both follow.  The engine calls the marcher in one configuration (contact_shadows.slang:63-71): jitter = 1, linear_march_exponent = 1,
 * bisection_steps = 0, use_secant = false, march_behind_surfaces = false, use_sloppy_march = false.  Only that configuration exists here;
 * the other branches of raymarch.slang are out of scope.  Per pixel (x, y) of the W x H depth image, size = float2(W, H):
 *   1. sky     depth == 0.0 gives 1.0 (a NaN depth is not sky).  Stated rule: the Slang marches such a pixel through 1 / 0.
 *   2. set-up  (contact_shadows.slang:45-61)  uv = (float2(x, y) + 0.5) / size;  cs = (uv * 2.0 - 1.0, depth);
 *              h = mul(inv_projection_view, (cs, 1)): h.r = ((M[r][0] * cs.x + M[r][1] * cs.y) + M[r][2] * cs.z) + M[r][3];  ws = h.xyz / h.w
 *              (the same operations in the same order as the unprojection of oxc_update_virtual_shadowmap's mark pass);
 *              ray = normalize(sun_dir) * shadow_length, once per call: l = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z), ray.k = (s.k / l) *
 *              shadow_length;  end_ws = ws + ray.
 *   3. ray end (raymarch.slang:559-568, 542-546, 502-537)  v = mul(view, (end_ws, 1)) (four rows, as h above);  p = mul(projection, v):
 *              p.r = ((P[r][0] * v.x + P[r][1] * v.y) + P[r][2] * v.z) + P[r][3] * v.w;  e = p.xyz / p.w;
 *              sign(a) = a > 0 ? 1.0 : a < 0 ? -1.0 : 0.0 (a NaN gives 0.0);  end = cs + (e - cs) * sign(e.z), per component.
 *              to_cs_dir_impl's perspective division has w = 1 + 0 * sign = 1 exactly (or NaN with e.z infinite, where end is NaN already):
 *              it divides by 1.0 and is omitted.
 *              Start clip: delta = end - cs;  near_edge.k = delta.k < 0 ? 1.0 : -1.0 for k = x, y (the Slang also computes z and does
 *              not use it: omitted);  m = max((near_edge.x - cs.x) / delta.x, (near_edge.y - cs.y) / delta.y);  start = cs + delta *
 *              max(0.0, m), three components.
 *              End clip: delta = end - start;  far_edge.k = delta.k >= 0 ? 1.0 : (k == z ? 0.0 : -1.0);  q.k = (far_edge.k - start.k) /
 *              delta.k, three components;  clip = min(1.0, min(min(q.x, q.y), q.z));  ray_end = start + delta * clip.
 *              A zero delta component divides by a signed zero; the IEEE result is the rule.  A pixel centre lies strictly inside the
 *              image, so for finite operands m is negative and start == cs.  delta.k == +0.0 gives -Inf in the start clip and +Inf in the
 *              end clip: that axis constrains neither.  delta.k == -0.0 would give m = +Inf and a NaN start (such a pixel ends as 1.0
 *              through the NaN rules below); end - cs of equal finite values is +0.0, so only a checker test reaches it.
 *   4. steps   (raymarch.slang:588-598)  cs_to_uv(c) = c * 0.5 + 0.5;  len_px = (cs_to_uv(ray_end.xy) - cs_to_uv(start.xy)) * size;
 *              n = max(2, min(steps, u32(floor(length(len_px))))), float -> u32 saturating, NaN -> 0;
 *              depth_thickness = thickness * (1.0 / near_clip), once per call.
 *   5. march   (raymarch.slang:123-175)  dir = ray_end - start;  for step = 0 .. n - 1, stopping at the first intersection:
 *              t = (f32(step) + 1.0) / f32(n)  (pow(v, 1.0) is v and lerp(0, 1, v) is v exactly: neither is evaluated);
 *              c = start + dir * t;  interp_uv = cs_to_uv(c.xy);  ray_depth = 1.0 / c.z.
 *   6. taps    (raymarch.slang:254-322)  Stated difference: the Slang's live branch samples with a hardware linear sampler, whose weights
 *              are fixed-point with an implementation-defined number of bits.  The rule is the Slang's own #else branch, the manual
 *              bilinear:  g = interp_uv * size - 0.5;  i = floor(g);  f = g - i;  the four texels (i.x + {0, 1}, i.y + {0, 1}), each
 *              coordinate clamped to [0, size - 1] (clamp to edge);  i is converted float -> i32 saturating, NaN -> 0, and i + 1 does
 *              not wrap: an i of INT_MAX reads the last column / row twice;
 *              bil = lerp(lerp(t00, t10, f.x), lerp(t01, t11, f.x), f.y)  (t10 is the texel at (i.x + 1, i.y));
 *              nearest = the texel at clamp(i32(floor(interp_uv * size)), 0, size - 1), the same conversion.
 *              linear_depth = 1.0 / bil;  unfiltered_depth = 1.0 / nearest;  max_depth = max(linear_depth, unfiltered_depth), min_depth =
 *              min(linear_depth, unfiltered_depth);  distance = max_depth * (1.0f + 0.000002f) - ray_depth, the factor rounded to binary32
 *              once (0x3F800011);  penetration = ray_depth - min_depth;  intersected = distance < 0.0 (a NaN distance is not).
 *   7. result  (raymarch.slang:617-623, contact_shadows.slang:73-77)  a hit = intersected && penetration < depth_thickness && distance <
 *              depth_thickness;  then frac = penetration / depth_thickness, smoothstep(1.0, 0.3, frac): s = min(max((frac - 1.0f) /
 *              (0.3f - 1.0f), 0.0), 1.0) with 0.3f - 1.0f evaluated in binary32 (0xBF333333), shadow = (s * s) * (3.0 - 2.0 * s);  the
 *              pixel is 1.0 - shadow.  Everything else (no intersection after n steps, or an intersection the thickness test rejects)
 *              is 1.0.
 * Rules the reference leaves open, decided here: the sampler's addressing of a coordinate outside the image or NaN is the clamp above;
 * the ray's sun-side normalisation and the thickness scale are evaluated once on the host, in the order shown; a texel of any bit pattern
 * (NaN, infinities, negative, denormal) goes through the same arithmetic -- max / min drop a NaN operand, every comparison with NaN is false.
 * Limits (else OXC_INVALID_ARG): depth_attachment and contact_shadows_attachment one R32F level each, of the same extent (at most 65536 a
 * side); steps in [1, 64]; thickness, shadow_length and near_clip finite and > 0; sun_dir finite and not the zero vector.  One launch, no
 * scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
typedef struct oxc_contact_shadows_context {
  uint32_t struct_size; /* sizeof(oxc_contact_shadows_context) */
  /* the GPU::Camera fields the pass reads */
  float inv_projection_view[16]; /* column-major, as view and projection */
  float view[16];
  float projection[16];
  float near_clip;
  /* the push constants (contact_shadows.slang:15-20) */
  float sun_dir[3];     /* towards the sun; normalised by the pass */
  uint32_t steps;
  float thickness;
  float shadow_length;
  oxc_image depth_attachment;           /* in: R32F, levels = 1, reversed Z, 0 = nothing drawn */
  oxc_image contact_shadows_attachment; /* out: R32F, levels = 1, the extent of the depth image */
} oxc_contact_shadows_context;

oxc_status oxc_contact_shadows(oxc_ctx* ctx, const oxc_contact_shadows_context* context, void* hip_stream);

/* ---- Ambient occlusion: the VBGTAO term from depth and normals -----------------------------------------------------
 * Replaces RendererInstance::generate_ambient_occlusion (Oxylus/src/Render/Passes/PBR.cpp:179-311), the call that follows the contact shadows
 * in RendererInstance::render (RendererInstance.cpp:1040-1055): the pipelines vbgtao_prefilter, vbgtao_main and vbgtao_denoise (passes/gtao/)
 * as three launches.  It fills the ambient_occlusion_attachment that pbr_apply reads.  Engine defaults: pp.vbgtao = 1, quality 3 ("ultra":
 * 9 slices x 3 samples per side; the four presets are 1 x 2, 2 x 2, 3 x 3, 9 x 3), GPU::VBGTAOSettings (SceneGPU.hpp:286-293): thickness 0.25,
 * effect_radius 0.5, noise_index 0, final_power 2.2.
 * Arithmetic: as oxc_resolve_shadowmap (binary32, round to nearest even, no contraction, IEEE division and square root, the Slang's evaluation
 * order; dot, length, normalize and cross as defined there; max / min are fmaxf / fminf: a NaN operand gives the other one; lerp(a, b, t) =
 * a + (b - a) * t; frac(x) = x - floor(x)); saturate(x) = min(max(x, 0), 1), so a NaN gives 0; sign(a) = a > 0 ? 1 : a < 0 ? -1 : 0 (NaN: 0);
 * float -> integer conversions saturate and NaN converts to 0; u32 -> f32 conversions are of values below 2^24 and exact; countbits is the
 * population count.  HALF_PI = 1.57079632679f, PI = 3.1415926535897932f, each rounded to binary32 once.  The reference is compiled fast-math
 * and samples through hardware gather and trilinear filtering, so it is not bit-defined: this is the one evaluation the device and the
 * checker (tests/ambient_occlusion_model.py) both follow.  No float operation of the per-pixel rules is reordered, contracted or approximated.
 * W x H is the extent of the depth image; level k of prefiltered_depth is max(1, W >> k) x max(1, H >> k).
 * Host evaluation, once per call, binary32, in this order:  (mul, add) = (projection[3][2], projection[2][2]) in glm indexing = elements 14
 *   and 10 of the column-major array (PBR.cpp:183-186);  the prefilter's radius r0 = (0.75f * 0.5f) * 1.457f;  for a radius r the falloff pair
 *   is falloff_range = 0.615f * r, falloff_from = r * (1.0f - 0.615f), falloff_mul = -1.0f / falloff_range, falloff_add = falloff_from /
 *   falloff_range + 1.0f (vbgtao_prefilter.slang:24-29 with r0, vbgtao_main.slang:157-161 with r = effect_radius * 1.457f);  far_thr =
 *   far_clip * 0.999f;  radius = ((0.5f * r) * |projection[0][0]|, (0.5f * r) * |projection[1][1]|);  f32(slice_count),
 *   f32(samples_per_slice_side);  noise_add = 288 * (noise_index % 64).  The divisions by projection[0][0] / [1][1] and by PI stay divisions,
 *   per evaluation.
 * Prefilter (vbgtao_prefilter.slang), one thread per 2 x 2 source texels, threads (bx, by) on a grid padded to multiples of 8:
 *   1. gather  (:57-58)  Stated rule: Gather at the corner of texel p0 = 2 * (bx, by) with offset (1, 1) names the integer texels .w = p0,
 *              .z = p0 + (1, 0), .x = p0 + (0, 1), .y = p0 + (1, 1), each coordinate clamped to [0, extent - 1].
 *   2. mip 0   (:19-21, :60-70)  linear = mul / (device_depth + add) for each of the four; each is stored at its own coordinate when that
 *              lies inside the image (odd extents: the clamped duplicates are computed and not stored).
 *   3. mip 1   (:23-39, :73-75)  weighted_average(d0 = .w, d1 = .z, d2 = .x, d3 = .y): m = min(min(d0, d1), min(d2, d3));  w_i =
 *              saturate((d_i - m) * falloff_mul + falloff_add);  total = ((w0 + w1) + w2) + w3;  result = ((((w0 * d0) + (w1 * d1)) +
 *              (w2 * d2)) + (w3 * d3)) / total.  Stored at (bx, by) when inside level 1.
 *   4. mips 2..4  (:79-115)  the thread with bx and by multiples of 2^(k-1) averages the level k - 1 values of the THREADS (bx, by),
 *              (bx + s, by), (bx, by + s), (bx + s, by + s), s = 2^(k-2), in that order, and stores at (bx, by) >> (k - 1) when inside
 *              level k.  A thread's value exists whether or not its own destination does: a destination texel outside a level is not
 *              written, and a 1-wide level's texel still averages the clamped values next to it.
 * Main (vbgtao_main.slang), one thread per pixel (x, y):
 *   5. edges   (:69-100)  Stated rule: the two GatherRed name the level-0 texels centre = (x, y), left = (x - 1, y), right = (x + 1, y), top =
 *              (x, y - 1), bottom = (x, y + 1), clamped.  e = (left, right, top, bottom) - centre;  slr = (e.y - e.x) * 0.5, stb = (e.w - e.z)
 *              * 0.5;  adj = e + (slr, -slr, stb, -stb);  e = min(|e|, |adj|);  e = saturate((1.0f + 0.25f) - e / (centre * 0.011f));
 *              depth_differences = packUnorm4x8(e): byte k = u32(floor(saturate(e_k) * 255.0f + 0.5f)) (a half-way value rounds up), component
 *              x in the low byte.  Written for every pixel.
 *   6. sky     (:171-174)  centre >= far_thr stores 1.0 (a NaN is not sky).  Otherwise linear_depth = centre * 0.99999f.
 *   7. set-up  (:59-67, :164, :176-188)  uv = (float2(x, y) + 0.5) / resolution;  view_position(uv, d) = (((uv.x * 2.0 - 1.0) / projection[0][0])
 *              * d, ((uv.y * 2.0 - 1.0) / projection[1][1]) * d, -d);  origin = view_position(uv, linear_depth);  view_dir = normalize(-origin);
 *              normal: Stated rule: the point sample is the normal texel at (x, y);  e = (.b, .a), binary16 -> binary32 exact with denormals
 *              kept;  n_w = oct_to_vec3(e) as in oxc_resolve_shadowmap step 2 (one normalisation);  normal = normalize(n_v), n_v.r = (V[r][0]
 *              * n_w.x + V[r][1] * n_w.y) + V[r][2] * n_w.z (the w = 0 term is left out);
 *              noise (:39-45): index = f32(hilbert_noise[y % 64][x % 64] + noise_add);  noise = frac(0.5f + index * (0.75487766624669276005f,
 *              0.5698402909980532659114f));
 *              screen_radius_uv = radius / linear_depth (both components);  min_s = 1.3f / max(screen_radius_uv.x * resolution.x, 1.3f).
 *   8. slice   (:191-208)  for slice_t = 0 .. slice_count - 1:  slice = (f32(slice_t) + noise.x) / f32(slice_count);  Stated difference:
 *              (c, s) = (cos, sin)(slice * PI) is the rotation rule of oxc_resolve_shadowmap step 6 applied to t = slice * 0.5f.  The zero
 *              component of direction = (c, s, 0) is left out of its products:  dv = c * view_dir.x + s * view_dir.y;  ortho = normalize((c -
 *              dv * view_dir.x, s - dv * view_dir.y, 0.0 - dv * view_dir.z));  axis = normalize((s * view_dir.z, -(c * view_dir.z), c *
 *              view_dir.y - s * view_dir.x));  pn = normal - axis * dot(normal, axis);  pnl = max(length(pn), 1e-6f);  sign_norm =
 *              sign(dot(ortho, pn));  n = sign_norm * fast_acos(saturate(dot(pn, view_dir) / pnl));  sample_mul = (c * screen_radius_uv.x,
 *              (-s) * screen_radius_uv.y).
 *              fast_acos(v) (:32-37): x = |v|;  res = -0.156583f * x + HALF_PI;  res = res * sqrt(saturate(1.0 - x));  v >= 0 ? res : PI - res.
 *   9. sample  (:212-231)  for sample_t = 0 .. samples_per_slice_side - 1:  sn = frac(noise.y + (f32(slice_t) + f32(sample_t) * f32(samples))
 *              * 0.6180339887498948482f);  s = (f32(sample_t) + sn) / f32(samples);  s = s * s;  s = s + min_s;  offset = s * sample_mul;
 *              p1 = uv + offset, p2 = uv - offset;  len = sqrt(q.x * q.x + q.y * q.y), q = offset * resolution;
 *              l = min(max(log2(len) - 3.30f, 0.0), 4.0), the log2 rule below.
 *              Stated difference (filtered samples): SampleLevel(linear clamp, p, l) is the manual bilinear of oxc_contact_shadows step 6
 *              (g = p * level_extent - 0.5, i = floor(g), f = g - i, four clamped texels, lerp(lerp(t00, t10, f.x), lerp(t01, t11, f.x), f.y))
 *              at level floor(l), giving a, and at level min(floor(l) + 1, 4), giving b;  depth = lerp(a, b, l - floor(l)).  Both levels are
 *              ALWAYS evaluated, also for a zero fraction: a non-finite texel of the second level then makes the sample NaN.
 *  10. arcs    (:124-146, :230-246)  delta = view_position(p, depth) - origin;  back = delta - view_dir * thickness;  h_f =
 *              fast_acos(dot(normalize(delta), view_dir)), h_b the same of back;  for side = +1 (p1) or -1 (p2): h = saturate((((side * -h)
 *              + n) + HALF_PI) / PI) for both;  (lo, hi) = side >= 0 ? (h_b, h_f) : (h_f, h_b).
 *              update_sectors (:102-119): angle = u32(ceil(saturate(hi - lo) * 32.0));  angle == 0 gives the empty mask;  start =
 *              min(u32(saturate(lo) * 32.0), 31);  mask = (0xFFFFFFFF >> (32 - angle)) << start, in 32 bits.
 *              falloff = saturate(length(delta) * falloff_mul + falloff_add);  occlusion += (falloff * f32(countbits(mask & ~bitmask))) / 32.0;
 *              bitmask |= mask;  side +1 first, then side -1.
 *  11. result  (:249-253)  per slice visibility += saturate(1.0 - occlusion);  ao = saturate(visibility / f32(slice_count)), stored in
 *              noisy_occlusion as binary16, round to nearest even, denormals kept.
 * Denoise (vbgtao_denoise.slang), one thread per pixel:
 *  12. taps    (:21-56)  Stated rule: the seven GatherRed name, clamped, the edge words of centre, left, right, top, bottom and the nine
 *              noisy values of the 3 x 3 neighbourhood (binary16 -> binary32, exact, denormals kept).  unpackUnorm4x8ToFloat: f32(byte k) /
 *              255.0f, (x, y, z, w) = (left, right, top, bottom) edge.  centre_edges *= (left.y, right.x, top.w, bottom.z);  the diagonal
 *              weights are 0.425f * (a * b + c * d) as the Slang writes them (:43-46).
 *  13. filter  (:58-81)  sum = centre * 1.2f, then += left, right, top, bottom, top-left, top-right, bottom-left, bottom-right value * weight
 *              in that order;  sum_weight likewise from 1.2f;  v = max(sum / sum_weight, 0.0);  out = pow(v, final_power), the pow rule
 *              below, stored as binary16 like step 11 (the reference's image is R16F).
 * log2 rule (stated difference: neither a library log2 nor v_log_f32 can be matched from numpy).  For binary32 x >= 2^-126: x = m * 2^e with m
 *   in [1, 2) from the bits;  m > 1.41421356f: m = m * 0.5 (exact), e = e + 1;  in binary64, no contraction: f = (double)m - 1.0, s = f / (2.0 +
 *   f), z = s * s, P = 1 + z (1/3 + z (1/5 + z (1/7 + z (1/9 + z (1/11 + z (1/13 + z (1/15 + z / 17))))))) by Horner with the binary64
 *   quotients 1.0 / k, L = (double)e + ((2.0 * s) * P) * 0x1.71547652b82fep+0;  log2(x) = L rounded to binary32 once.  x < 2^-126 (zero,
 *   denormal, negative) and NaN give -Inf; +Inf gives +Inf.  Within 2^-23 relative (2^-24 absolute below 1) of the exact value
 *   (tests/test_ambient_occlusion_model.py).
 * pow rule, for v >= 0 and final_power p > 0:  y = (double)p * L(v), L the binary64 value above before its rounding;  k = floor(y + 0.5), r =
 *   y - k (exact), t = r * 0x1.62e42fefa39efp-1, E = sum_{n = 0..13} t^n / n! by Horner with the binary64 quotients 1.0 / n!;  pow = E * 2^k
 *   rounded to binary32 once.  y <= -160 gives 0.0 and y >= 160 gives +Inf (what the rounding would give).  pow(0, p) = 0.0 (v below 2^-126
 *   likewise) and pow(1, p) = 1.0 exactly.
 * Rules the reference leaves open, decided here: a texel of any bit pattern goes through the same arithmetic; the kernels run with the FP16
 * denormal mode at its default (denormals kept), unlike the cull kernels.
 * Limits (else OXC_INVALID_ARG, nothing written): depth_attachment one R32F level at offset 0, at most 65536 a side; prefiltered_depth of the
 * same extent with exactly 5 levels at 4-byte aligned offsets; normal_attachment 8-byte aligned with one u16x4 per pixel; hilbert_noise
 * u16[64][64], 2-byte aligned; depth_differences 4-byte aligned u32 per pixel; noisy_occlusion and ambient_occlusion_attachment 2-byte
 * aligned u16 per pixel; slice_count in [1, 16], samples_per_slice_side in [1, 8]; thickness, effect_radius, final_power, far_clip and both
 * components of resolution finite and > 0; noise_index any value.  The three intermediates are caller-owned; the context's arena is not
 * touched.  Three launches, no allocation, no host synchronisation; capturable into a HIP graph.  Every pixel of every output is written. */
typedef struct oxc_ambient_occlusion_context {
  uint32_t struct_size; /* sizeof(oxc_ambient_occlusion_context) */
  /* the GPU::Camera fields the pass reads */
  float view[16];       /* column-major, as projection */
  float projection[16];
  float resolution[2];
  float far_clip;
  /* GPU::VBGTAOSettings (SceneGPU.hpp:286-293), same order and types */
  float thickness;
  uint32_t slice_count;
  uint32_t samples_per_slice_side;
  float effect_radius;
  uint32_t noise_index;
  float final_power;
  oxc_image depth_attachment;              /* in: R32F, levels = 1, reversed Z */
  oxc_buffer normal_attachment;            /* in: u16x4[height][width], only .b and .a are read (as in oxc_shadow_resolve_context) */
  oxc_buffer hilbert_noise;                /* in: u16[64][64], the engine's Hilbert index table (RendererInstance.cpp:150-177) */
  oxc_image prefiltered_depth;             /* out, caller-owned: R32F, exactly 5 levels, linear view-space depth */
  oxc_buffer depth_differences;            /* out, caller-owned: u32[height][width], the packed edges */
  oxc_buffer noisy_occlusion;              /* out, caller-owned: binary16 as u16[height][width] */
  oxc_buffer ambient_occlusion_attachment; /* out: binary16 as u16[height][width] */
} oxc_ambient_occlusion_context;

oxc_status oxc_generate_ambient_occlusion(oxc_ctx* ctx, const oxc_ambient_occlusion_context* context, void* hip_stream);

/* ---- terrain patch cull ---------------------------------------------------------
 * Replaces RendererInstance::cull_terrain (Oxylus/src/Render/Passes/Terrain.cpp:159-216) + pipeline
 * terrain_cull (Shaders/passes/terrain_cull.slang:17-83): one thread per patch, world-space AABB from the
 * patch grid and the patch_minmax image, the same test_frustum / project_aabb / test_occlusion and early/late
 * mask protocol as cull_meshlets_hiz, survivors appended to visible_patches and counted in
 * DrawIndirectCommand.instance_count.  The reference appends in atomic order; here the list is ascending. */
typedef struct oxc_terrain_context {
  uint32_t struct_size;
  uint32_t cull_flags;               /* OXC_CULL_* (TestFrustum, TestOcclusion, LatePass) */
  oxc_cull_camera cull_camera;       /* projection_view, near_clip; mesh_instance_count is set by the callee (Terrain.cpp:171) */
  /* the GPU::TerrainData fields the shader reads (SceneGPU.hpp:440-453, scene.slang:634-661) */
  float world_min[2];
  float world_size[2];
  uint32_t patch_count[2];
  float base_height;
  float height_scale;
  oxc_image patch_minmax_attachment; /* RG32F, patch_count.x x patch_count.y, levels = 1: {min, max} normalised height per patch */
  oxc_image hiz_attachment;          /* read when TestOcclusion or LatePass */
  oxc_buffer visible_patches_buffer; /* out: u32[patch_total] */
  oxc_buffer patch_visibility_mask_buffer; /* in/out: u32[ceil(patch_total / 32)] */
  oxc_buffer draw_cmd_buffer;        /* out (callee-owned, like the reference's scratch_buffer): VkDrawIndirectCommand {4, instance_count, 0, 0} */
} oxc_terrain_context;

oxc_status oxc_cull_terrain(oxc_ctx* ctx, oxc_terrain_context* context, void* hip_stream);

/* ---- consumer of the indirect draw ------------------------------------------------
 * What RendererInstance::draw_for_visbuffer does with cull_geometry's outputs (Passes/DrawGeometry.cpp:104-190,
 * pipeline visbuffer_encode, passes/visbuffer_encode.slang:24-49; cullMode eBack, depth GreaterOrEqual,
 * reversed Z), as a compute rasteriser -- so that early cull -> draw -> depth -> generate_hiz -> late cull -> draw
 * runs without a graphics queue.  The fixed-function rasteriser's sample rules cannot be matched bit for bit;
 * the rules used instead are stated here and in the checker:
 *   vertex  VisBufferData(index) -> (meshlet instance, corner); Meshlet::index, Mesh::decode_position;
 *           world = mul(world, (p,1)).xyz, clip = mul(projection_view, (world,1))              (as vs_main);
 *   clip    Sutherland-Hodgman against five planes in this order: w >= 2^-10, 64 w - x >= 0, 64 w + x >= 0, 64 w - y >= 0,
 *           64 w + y >= 0 (a 64x guard band: every screen coordinate stays inside the +-2^20 px fixed-point range for extents up
 *           to 16384; the reference's fixed-function clipper stands here).  A vertex with distance d >= 0 is inside.  On a crossing
 *           edge with inside end I and outside end O the new vertex is I + t (O - I), t = d(I) / (d(I) - d(O)), binary32, no
 *           contraction, all four clip coordinates -- the same value for both triangles that share the edge.  The polygon
 *           (<= 8 corners) is drawn as the fan (p0, pk, pk+1), each with the vis value of the source triangle; a triangle inside
 *           every plane is untouched (round 1 had no clipper and dropped triangles with a corner at w <= 0).  Capacity: the
 *           ids of the triangles that cross a plane are queued, 2^22 per call; when more cross, an overflow pass walks the index
 *           list again and clips every crossing triangle it finds (slow, and the same image: drawing a triangle twice changes nothing);
 *   setup   screen = (clip.xy / clip.w * 0.5 + 0.5) * extent, snapped to 1/256 pixel; back faces (fixed-point
 *           area >= 0, the orientation cull_triangles' determinant test calls back-facing) are dropped;
 *   cover   pixel centres, integer edge functions, top-left rule;
 *   depth   z/w interpolated in binary64, ((e0 z0 + e1 z1) + e2 z2) * (1 / area) with the exact integer edge values e_i, rounded to
 *           binary32, kept when in (0, 1];
 *           per pixel the maximum of (depth bits << 32) | vis wins (64-bit atomic max), vis = (instance << 8) |
 *           (corner / 3) as VisBufferData::encode -- order-independent: one of the results the reference's
 *           equal-depth race can produce.
 * `visdepth_buffer` (u64[width * height]) persists between the early and the late draw of a frame; `clear` zeroes
 * it first.  `depth_attachment` (R32F, levels = 1) and `visbuffer_attachment` (u32) are optional resolves. */
typedef struct oxc_draw_context {
  uint32_t struct_size;
  uint32_t wide_triangle_index; /* same meaning as in oxc_cull_geometry_context */
  uint32_t clear;
  uint32_t width, height;
  uint32_t _pad;
  float projection_view[16];           /* Camera::projection_view, column-major */
  oxc_buffer draw_geometry_cmd_buffer; /* from oxc_cull_geometry: indexCount is read on the device */
  oxc_buffer visdepth_buffer;
  oxc_image depth_attachment;          /* optional out */
  oxc_buffer visbuffer_attachment;     /* optional out */
} oxc_draw_context;

oxc_status oxc_draw_visbuffer(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_draw_context* context, void* hip_stream);

/* ---- Visbuffer decode: the G-buffer images from the visibility buffer --------------------------------------------------
 * Replaces RendererInstance::decode_visbuffer (Oxylus/src/Render/Passes/DrawGeometry.cpp:192-274, pipeline visbuffer_decode, passes/
 * visbuffer_decode.slang), the full-screen pass directly after the draw (RendererInstance.cpp:924): per pixel the visbuffer texel is turned
 * back into a triangle, the perspective-correct barycentrics are found, the vertex normals are interpolated, and the four G-buffer images
 * every later pass reads are written (formats: RendererInstance.cpp:700-737).  Its normal_attachment is what oxc_resolve_shadowmap and
 * oxc_generate_ambient_occlusion read.
 * Scope: the geometry and material-factor half of the shader.  Texture sampling is NOT done -- bindless images, SampleGrad and anisotropy
 * are hardware rules this library has no image table for: the Has*Image bits of Material::flags are ignored, every sample_* returns its
 * factor alone (scene.slang:110-159 without the image branches), sample_occlusion_color is 1.0, normal.xy equals normal.zw, and what feeds
 * only the sampling -- uv_size, uv_offset, the texcoord stream, the tangent frame, the rescaled ddx / ddy of compute_partial_derivatives
 * (visbuffer_decode.slang:74-83) -- is not computed.  Camera::position is read by the Slang for the tangent frame only; the context has no
 * such field.  Terrain pixels and the mesh-shader path are out of scope.  oxc_decode_visbuffer_textured (below) is the pass with an
 * image table and everything left out here.
 * Arithmetic: canonical binary32 -- round to nearest even, one fixed evaluation order, no contraction, IEEE division and square root; 1.0 / x
 * is a division; sums run left to right as written in the Slang; mul(M, (p, 1)).r = ((M[r][0] * p.x + M[r][1] * p.y) + M[r][2] * p.z) +
 * M[r][3]; mul(vec, mat) is the dot product in component order; saturate(x) = min(max(x, 0), 1) with fmaxf / fminf, so a NaN gives 0.  The
 * reference is compiled fast-math: this is the one evaluation the device and the checker (tests/visbuffer_decode_model.py) both follow.
 * Per pixel (x, y) of the W x H images:
 *   1. empty   (visbuffer_decode.slang:90-93)  The pixel is empty when texel == ~0u, or is_terrain(texel) ((texel >> 8) == 0xFFFFFE,
 *              visbuffer.slang:16-20), or the bits of the depth texel are 0 (the library's own cleared state: oxc_draw_visbuffer resolves an
 *              uncovered pixel to vis 0 and depth 0), or meshlet_instance_index = texel >> 8 is >= meshlet_instance_count (the reference
 *              would read past the buffer).  With clear != 0 the four outputs of an empty pixel are written as zero (the engine's
 *              clear_image to black, folded in); with clear == 0 they are not touched.
 *   2. fetch   (visbuffer_decode.slang:95-110)  VisBufferData(texel): triangle_index = texel & 0xFF.  meshlet_instance -> mesh_instance ->
 *              mesh, material_index, transform, mesh.lods[lod_index] -> meshlet; Meshlet::indices (scene.slang:365-376): the three micro
 *              indices at bytes local_triangle_index_offset + 3 * triangle_index + {0, 1, 2} of local_triangle_indices (get_micro_index reads
 *              the u32 word that holds the byte), then indirect_vertex_indices[indirect_vertex_index_offset + micro].  If any of the three
 *              vertex indices exceeds vertex_count - 1 (unsigned: vertex_count == 0 wraps and nothing exceeds it, as in the Slang), all four
 *              outputs are written as zero -- written, not discarded, also with clear == 0.  material_index >= material_count uses a default
 *              Material, all fields zero.  Only meshlet_instance_index and material_index are bounded by the call; every other index of the
 *              chain is the scene's own, as everywhere in this library.
 *   3. vertex  positions through com::dequantize_half (Mesh::decode_position, scene.slang:478-484): a half with exponent field 0 gives the
 *              sign alone (+-0), every other half its IEEE value; the material's halves likewise.  Normals through Mesh::decode_normal
 *              (scene.slang:486-489): (f32((packed >> {20, 10, 0}) & 1023) / 511.0) - 1.0.  A null Mesh::vertex_normals decodes every normal
 *              as (0, 0, 0) and the arithmetic runs on (stated rule: the Slang would read through the null pointer).
 *   4. bary    (visbuffer_decode.slang:45-73)  world_i = mul(world, (p_i, 1)).xyz (TransformWorld::to_world_positions); clip_i =
 *              mul(projection_view, (world_i, 1)) (x, y and w are used);  inv_w_i = 1.0 / clip_i.w;  ndc_i = clip_i.xy * inv_w_i;
 *              inv_det = 1.0 / ((ndc_2.x - ndc_1.x) * (ndc_0.y - ndc_1.y) - (ndc_2.y - ndc_1.y) * (ndc_0.x - ndc_1.x));
 *              ddx = ((ndc_1.y - ndc_2.y, ndc_2.y - ndc_0.y, ndc_0.y - ndc_1.y) * inv_det) * inv_w, ddy = ((ndc_2.x - ndc_1.x, ndc_0.x -
 *              ndc_2.x, ndc_1.x - ndc_0.x) * inv_det) * inv_w, per component;  ddx_sum = (ddx.x + ddx.y) + ddx.z, ddy_sum likewise;
 *              uv = ((f32(x) + 0.5) / f32(W), (f32(y) + 0.5) / f32(H)) * 2.0 - 1.0 (the fullscreen triangle's tex_coord: the pixel-centre rule
 *              of the other per-pixel passes);  d = uv - ndc_0;  interp_inv_w = (inv_w_0 + d.x * ddx_sum) + d.y * ddy_sum;  interp_w = 1.0 /
 *              interp_inv_w;  lambda = (interp_w * ((inv_w_0 + d.x * ddx.x) + d.y * ddy.x), interp_w * (d.x * ddx.y + d.y * ddy.y),
 *              interp_w * (d.x * ddx.z + d.y * ddy.z)).  A zero-area triangle divides by zero; the IEEE results are the rule.
 *   5. normal  (visbuffer_decode.slang:136-137, 169-170)  N = TransformWorld::normal_matrix() (scene.slang:292-299: the cofactor matrix of
 *              world's upper 3 x 3, each entry a * b - c * d with both products rounded);  n_i = mul(N, normal_i) row by row;  v.c =
 *              (lambda.x * n_0.c + lambda.y * n_1.c) + lambda.z * n_2.c;  world_normal = v / sqrt((v.x * v.x + v.y * v.y) + v.z * v.z), three
 *              divisions;  vec3_to_oct (common/encoding.slang:17-21): s = 1.0 / ((|x| + |y|) + |z|), p = (x * s, y * s), and for z <= 0
 *              ((1.0 - |p.y|) * (p.x >= 0 ? 1 : -1), (1.0 - |p.x|) * (p.y >= 0 ? 1 : -1)), else p.  Both .rg and .ba of normal_attachment
 *              get it, converted to binary16 with round to nearest even, denormals kept.  Stated rule: a NaN component is stored as 0x7E00
 *              whatever its sign and payload (IEEE leaves both open, and processors differ).
 *   6. albedo  (scene.slang:67-74, 110-119)  the four dequantized halves of albedo_color;  each of r, g, b through the sRGB encoding x <=
 *              0.0031308f ? 12.92f * x : 1.055f * pow(x, 1.0f / 2.4f) - 0.055f, the exponent rounded to binary32 once (0x3ED55555) and pow
 *              the closed form of oxc_generate_ambient_occlusion (above; a NaN or negative x ends as 0 through saturate, +Inf as 255);
 *              alpha stays linear;  every channel is u32(floor(saturate(c) * 255.0f + 0.5f)), R in the low byte.
 *   7. m/r/o   metallic_roughness_occlusion = (metallic_factor, roughness_factor, 1.0, 0.0) by the same unorm8 rule, metallic in the low byte.
 *   8. emissive  the three dequantized halves of emissive_color packed as UF11 (bits 0-10), UF11 (11-21), UF10 (22-31): 5 exponent bits
 *              (bias 15) and 6 / 5 mantissa bits.  The Vulkan specification leaves the rounding open; the rule, for the binary32 value:
 *              NaN gives exponent 31 with an all-ones mantissa; negative values, -0 and -Inf give 0; +Inf gives exponent 31, mantissa 0; a
 *              value at or above 2^16 gives the largest finite pattern (exponent 30, all-ones mantissa); otherwise the exponent is re-biased
 *              and the mantissa truncated toward zero, and below 2^-14 the small format's denormals are kept (truncated likewise).
 * Limits (else OXC_INVALID_ARG, nothing launched): width and height not zero and equal to the depth attachment's (at most 65536 a side);
 * depth_attachment one R32F level at offset 0; visbuffer_attachment, albedo_attachment, emissive_attachment and
 * metallic_roughness_occlusion_attachment 4-byte aligned with one u32 per pixel; normal_attachment 8-byte aligned with one u16x4 per pixel;
 * materials_buffer 4-byte aligned with material_count records of 56 bytes (may be null when material_count is 0); the frame's meshes,
 * transforms (16-byte aligned), mesh_instances and meshlet_instances buffers not null, the last holding meshlet_instance_count records.  A
 * MeshLOD's local_triangle_indices must be allocated in whole u32 words (its byte count rounded up to a multiple of 4): get_micro_index loads
 * the word that holds a byte, as the Slang and oxc_draw_visbuffer do, so the last word is read even when the stream ends inside it.  One
 * launch, no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
typedef struct oxc_decode_context {
  uint32_t struct_size; /* sizeof(oxc_decode_context) */
  uint32_t width, height;
  uint32_t clear;                  /* != 0: empty pixels are written as zero */
  uint32_t meshlet_instance_count; /* records of frame->meshlet_instances_buffer a texel may name */
  uint32_t material_count;
  float projection_view[16];       /* Camera::projection_view, column-major: the matrix the visbuffer was drawn with */
  oxc_buffer visbuffer_attachment; /* in: u32[height][width], as oxc_draw_visbuffer resolves it */
  oxc_image depth_attachment;      /* in: R32F, levels = 1, as oxc_draw_visbuffer resolves it */
  oxc_buffer materials_buffer;     /* in: GPU::Material[material_count], 56 bytes each (SceneGPU.hpp:67-82) */
  oxc_buffer albedo_attachment;    /* out: R8G8B8A8 sRGB, u32[height][width], R in the low byte */
  oxc_buffer normal_attachment;    /* out: R16G16B16A16 Sfloat, u16x4[height][width], the layout oxc_resolve_shadowmap reads */
  oxc_buffer emissive_attachment;  /* out: B10G11R11 UfloatPack32, u32[height][width] */
  oxc_buffer metallic_roughness_occlusion_attachment; /* out: R8G8B8A8 Unorm, u32[height][width] */
} oxc_decode_context;

/* meshlet_instances, mesh_instances, meshes and transforms come from `frame`, as in oxc_draw_visbuffer. */
oxc_status oxc_decode_visbuffer(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_decode_context* context, void* hip_stream);

/* ---- Textured visbuffer decode: the same pass with the five material images sampled ------------------------------------------
 * The whole of passes/visbuffer_decode.slang: what oxc_decode_visbuffer leaves out -- the texcoord stream, uv_size / uv_offset, the
 * rescaled ddx / ddy (visbuffer_decode.slang:74-83), the tangent frame (:128-151), SampleGrad of the albedo, normal, emissive,
 * metallic-roughness and occlusion images (scene.slang:110-159) and the normal map (:153-167).  oxc_decode_visbuffer does not change; this
 * entry takes its context, with the same limits and the same four outputs, and an image table.
 * A hardware sampler's fixed-point weights, LOD approximation and anisotropy are implementation-defined; as for the bilinear of
 * oxc_apply_bloom, the trilinear of oxc_generate_ambient_occlusion and the repeat axis of oxc_apply_tonemap, the rule here is a stated
 * one in the canonical binary32 of oxc_decode_visbuffer (round to nearest even, evaluation in the order written, no contraction, IEEE
 * division and square root) that the device and the checker (tests/textured_decode_model.py) both follow.  Stated differences from a
 * Vulkan sampler: weights are binary32, not 8-bit fixed point; lambda is the closed-form log2 of the exact rho, not an approximation;
 * LinearSamplerRepeatedAnisotropy is sampled as linear / repeat / linear-mip -- anisotropic filtering is not attempted.
 * Out of scope: block-compressed formats; mip generation (the caller supplies every level); the alpha test of the draw (alpha_cutoff
 * is not read); the mesh-shader path.
 * Image formats: OXC_IMAGE_R8G8B8A8_UNORM (channel = f32(byte) / 255.0f), OXC_IMAGE_R8G8B8A8_SRGB (r, g, b = srgb_decode(byte) of
 * oxc_apply_pbr step 2; alpha = f32(byte) / 255.0f) and OXC_IMAGE_R8G8_UNORM (r, g as Unorm, b = 0, a = 1: NormalTwoComponent maps).  R is
 * the lowest byte of a texel.  Level k of an image is max(1, width >> k) x max(1, height >> k) texels, row-major, tightly packed, at
 * dptr + level_offset[k]; a side is at most 16384 and an image has at most 15 levels (a larger `levels` is taken as 15).
 * Sampler records: filter 0 nearest / 1 linear, address 0 repeat / 1 clamp to edge, mip_filter 0 nearest / 1 linear; any other value of
 * a field is taken as 1.  The five SamplingMode presets of Renderer.cpp:64-70: LinearRepeated {1, 0, 1}, LinearClamped {1, 1, 1}, NearestRepeated
 * {0, 0, 0}, NearestClamped {0, 1, 0}, LinearRepeatedAnisotropy {1, 0, 1}.
 * Per pixel, steps 1 - 5 of oxc_decode_visbuffer unchanged (step 2 reads the whole 14-word Material; the default Material is all zero:
 * no flag set).  Then:
 *   9. texcoords  (Mesh::decode_texcoord, scene.slang:491-497)  t_i = (dequantize_half(packed.x), dequantize_half(packed.y)) of
 *              texture_coords[vertex_i], x in the low half, by the flushing dequantize_half of step 3.  A null Mesh::texture_coords
 *              decodes every texcoord as (0, 0).
 *  10. gradients (visbuffer_decode.slang:74-83, 32-39, 119-122)  two_over_resolution = (2.0 / f32(W), 2.0 / f32(H));  sx =
 *              two_over_resolution.x, sy = -two_over_resolution.y;  ddx' = ddx * sx, ddy' = ddy * sy per component, ddx_sum' = ddx_sum * sx,
 *              ddy_sum' = ddy_sum * sy (ddx, ddy and the sums of step 4);  interp_ddx_w = 1.0 / (interp_inv_w + ddx_sum'), interp_ddy_w =
 *              1.0 / (interp_inv_w + ddy_sum');  ddx''.c = interp_ddx_w * (lambda.c * interp_inv_w + ddx'.c) - lambda.c, ddy''.c =
 *              interp_ddy_w * (lambda.c * interp_inv_w + ddy'.c) - lambda.c.  gradient_of: uv.c = (lambda.x * t_0.c + lambda.y * t_1.c) +
 *              lambda.z * t_2.c, uv_ddx.c = (ddx''.x * t_0.c + ddx''.y * t_1.c) + ddx''.z * t_2.c, uv_ddy likewise.  Then with uv_size and
 *              uv_offset through dequantize_half: uv.c = uv.c * uv_size.c + uv_offset.c, uv_ddx.c = uv_ddx.c * uv_size.c, uv_ddy.c =
 *              uv_ddy.c * uv_size.c.
 *  11. tangent frame (:128-151), computed where a normal image is sampled.  r_i = world_i - camera_position per component;  pos_ddx.c =
 *              (ddx''.x * r_0.c + ddx''.y * r_1.c) + ddx''.z * r_2.c, pos_ddy likewise;  dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z;
 *              N = world_normal of step 5;  pos_ddx_s.c = pos_ddx.c - dot(pos_ddx, N) * N.c, pos_ddy_s likewise;  jacobian_sign =
 *              sign(uv_ddx.x * uv_ddy.y - uv_ddx.y * uv_ddy.x) with sign(NaN) = 0 and sign(+-0) = 0;  T.c = jacobian_sign * (uv_ddy.y *
 *              pos_ddx_s.c - uv_ddx.y * pos_ddy_s.c), normalised by step 5's normalize (sqrt, three divisions) only when jacobian_sign != 0;
 *              w = jacobian_sign * sign(dot(pos_ddy, cross(N, pos_ddx)));  B.c = (-w) * cross(N, T).c;  cross(a, b).x = a.y * b.z - a.z *
 *              b.y and its rotations.
 *  12. SampleGrad, one rule for all five images, of image (width, height, levels) under the material's sampler:
 *              LOD.  mx = (uv_ddx.x * f32(width), uv_ddx.y * f32(height)), my likewise from uv_ddy;  rho = fmaxf(sqrt(mx.x * mx.x + mx.y *
 *              mx.y), sqrt(my.x * my.x + my.y * my.y)) (fmaxf: a NaN loses to a number);  lambda = (float)log2_f64(rho), the closed form of
 *              oxc_generate_ambient_occlusion before its rounding (zero, a denormal, a negative value and NaN give -Inf);  a NaN lambda is
 *              taken as 0;  lambda = fminf(fmaxf(lambda, 0), f32(levels - 1)).  Linear mips: lo = (int)floor(lambda), hi = min(lo + 1,
 *              levels - 1); both levels are always tapped; result.c = lerp(tap_lo.c, tap_hi.c, lambda - floor(lambda)), lerp(a, b, t) = a +
 *              (b - a) * t.  Nearest mips: the one level min((int)floor(lambda + 0.5f), levels - 1).
 *              Level tap of a w x h level at uv.  Linear filter, per axis with coordinate p and side n: repeat is the repeat axis of
 *              oxc_apply_tonemap (g = p * f32(n) - 0.5, i0 = floor_mod(the saturating conversion of floor(g), n), i1 = i0 + 1 wrapped to 0,
 *              f = g - floor(g)); clamp is the clamp axis of oxc_apply_bloom (i0 and i1 = i and i + 1 clamped to [0, n - 1]).  The four
 *              texels are decoded first, then combined per channel in the bloom's order: lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy).
 *              Nearest filter: the texel at i = the saturating conversion of floor(p * f32(n)), floor_mod(i, n) under repeat, clamped to
 *              [0, n - 1] under clamp.  A NaN coordinate converts to texel 0, +-Inf saturates to INT_MAX / INT_MIN before the wrap or the
 *              clamp, and a coordinate beyond int32 likewise: every tap reads inside its level for every bit pattern of uv.
 *  13. bounds  An image whose Has*Image flag is set is "absent" when its index is >= image_count, or its record has levels == 0, a null
 *              dptr, a format above 2 or a side of 0 or above 16384: nothing of it is read and the result is that of a clear flag.  A
 *              sampler_index >= sampler_count samples as linear / repeat / linear-mip.  The one sampler_index serves all five images.
 *  14. outputs  albedo = albedo_factor * texel in all four channels, then step 6.  Normal, when the normal image is present: s = texel.rgb *
 *              2.0 - 1.0 per channel;  NormalFlipY: s.y = -s.y;  NormalTwoComponent: s.z = sqrt(saturate(1.0 - (s.x * s.x + s.y * s.y)));
 *              n.c = (s.x * T.c + s.y * B.c) + s.z * N.c, normalised as in step 5;  normal.rg = vec3_to_oct(n).  normal.ba is always
 *              vec3_to_oct(world_normal), the bytes oxc_decode_visbuffer writes; without a normal image .rg equals .ba.  emissive = factor *
 *              texel.rgb, then step 8.  (metallic, roughness) = (metallic_factor * texel.b, roughness_factor * texel.g);  occlusion =
 *              texel.r of the occlusion image, 1.0 without one;  then step 7.  With no image flag set (or every flagged image absent) all
 *              four outputs are oxc_decode_visbuffer's, byte for byte.
 * Limits (else OXC_INVALID_ARG, nothing launched): those of oxc_decode_visbuffer; images->struct_size; images_buffer not null, 8-byte
 * aligned and image_count * 144 bytes when image_count != 0; samplers_buffer not null, 4-byte aligned and sampler_count * 16 bytes when
 * sampler_count != 0.  With a count of 0 its buffer is not looked at.  The image records live on the device and the host cannot validate
 * them: beyond step 13 the scene owns their correctness (level offsets inside the allocation, R8G8B8A8 levels 4-byte aligned, R8G8 levels
 * 2-byte aligned), as it does for the mesh chain.  One launch, 2 KiB of LDS, no scratch, no allocation, no host synchronisation;
 * capturable into a HIP graph. */
enum { OXC_IMAGE_R8G8B8A8_UNORM = 0, OXC_IMAGE_R8G8B8A8_SRGB = 1, OXC_IMAGE_R8G8_UNORM = 2 };
enum { OXC_FILTER_NEAREST = 0, OXC_FILTER_LINEAR = 1 };
enum { OXC_ADDRESS_REPEAT = 0, OXC_ADDRESS_CLAMP_TO_EDGE = 1 };

typedef struct oxc_material_image { /* device record, 144 bytes */
  uint64_t dptr;
  uint32_t width, height, levels, format;
  uint64_t level_offset[15]; /* bytes from dptr */
} oxc_material_image;

typedef struct oxc_material_sampler { /* device record, 16 bytes */
  uint32_t filter, address, mip_filter, _pad;
} oxc_material_sampler;

typedef struct oxc_material_images {
  uint32_t struct_size;     /* sizeof(oxc_material_images) */
  float camera_position[3]; /* Camera::position: the tangent frame reads it */
  uint32_t image_count;
  uint32_t sampler_count;
  oxc_buffer images_buffer;   /* in: oxc_material_image[image_count]: what Material::*_image_index name (the engine's global_images) */
  oxc_buffer samplers_buffer; /* in: oxc_material_sampler[sampler_count]: what Material::sampler_index names (global_samplers) */
} oxc_material_images;

oxc_status oxc_decode_visbuffer_textured(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_decode_context* context,
                                         const oxc_material_images* images, void* hip_stream);

/* ---- PBR apply: the lit HDR image from the G-buffer and the shadow terms --------------------------------------------------
 * Replaces the no-atmosphere branch of RendererInstance::apply_pbr (Oxylus/src/Render/Passes/PBR.cpp:313-534, the else branch from :435,
 * pipeline pbr_apply_no_atmos, passes/pbr_apply_no_atmos.slang with pbr.slang), the full-screen pass that reads what oxc_decode_visbuffer,
 * oxc_resolve_shadowmap, oxc_contact_shadows and oxc_generate_ambient_occlusion wrote and the first one whose output is a picture.
 * Out of scope: the atmosphere branch (passes/pbr_apply.slang: the sky LUTs, the cubemap, aerial perspective), which is
 * oxc_apply_pbr_atmosphere below -- here scene_flags with OXC_SCENE_HAS_ATMOSPHERE is OXC_INVALID_ARG; tone mapping and the other post passes; tiled or clustered light culling (the reference
 * has none); any change to what the five producer passes write.
 * Arithmetic: the canonical binary32 arithmetic of the other passes -- round to nearest even, one fixed order, no contraction, IEEE division
 * and square root; 1.0 / x is a division; min, max, clamp and saturate go through fmaxf / fminf, so a NaN operand loses (saturate(NaN) = 0,
 * clamp(x, lo, hi) = min(max(x, lo), hi)); sums and dot products run left to right as written in the Slang (dot(a, b) = (a.x * b.x + a.y *
 * b.y) + a.z * b.z); a product of three factors a * b * c is (a * b) * c; lerp(a, b, t) = a + (b - a) * t; reflect(i, n) = i - (2.0 * dot(n,
 * i)) * n; length(v) = sqrt(dot(v, v)), normalize(v) = v / length(v) (three divisions), smoothstep(e0, e1, x): s = saturate((x - e0) / (e1 -
 * e0)), (s * s) * (3.0 - 2.0 * s), as oxc_contact_shadows states them.  PI = 3.1415926535897932f rounded to binary32 once; Fd_Lambert() =
 * 1.0f / PI, one binary32 division.  A comparison with a NaN operand is false.  The reference is compiled fast-math and reads its images
 * through samplers: this is the one evaluation the device and the checker (tests/pbr_apply_model.py) both follow.
 * Per pixel (x, y) of the W x H images:
 *   1. transparent  (:34-38)  depth = the depth texel.  With OXC_SCENE_TRANSPARENT_BACKGROUND and depth == 0.0 all four channels are 0 and the
 *              pixel is done (class "transparent empty").
 *   2. decode  (:40-54)  albedo: Stated rule: the linear sampler at the pixel centre is, in exact arithmetic, the texel itself: a load of
 *              texel (x, y).  Bytes R, G, B (R in the low byte; alpha is not read) through the sRGB decode c = f32(byte) / 255.0f;  c <=
 *              0.04045f ? c / 12.92f : pow((c + 0.055f) / 1.055f, 2.4f), pow the pow rule of oxc_generate_ambient_occlusion with the exponent
 *              rounded to binary32 once (256 possible results).  normal: the four halves through binary16 -> binary32, exact, denormals kept;
 *              mapped = oct_to_vec3(.rg), smooth = oct_to_vec3(.ba), oct_to_vec3 as in oxc_resolve_shadowmap step 2 (one normalisation
 *              inside).  emission: UF11 (bits 0-10), UF11 (11-21), UF10 (22-31) decoded exactly -- exponent field 0: mantissa * 2^-(14 + M),
 *              1..30: (1 + mantissa / 2^M) * 2^(e - 15), 31: +Inf for a zero mantissa, NaN otherwise (M = 6 or 5 mantissa bits); every
 *              pattern is a binary32 value.  metallic_roughness_occlusion: bytes 0, 1, 2 as f32(byte) / 255.0f;  metallic = clamp(.r, 0.0,
 *              1.0);  roughness = clamp(.g, 0.045f, 1.0);  occlusion = .b * ao, ao the ambient-occlusion half (binary16 -> binary32, exact,
 *              denormals kept).
 *   3. position  (:56-58)  uv = ((f32(x) + 0.5) / f32(W), (f32(y) + 0.5) / f32(H));  NDC = (uv * 2.0 - 1.0, depth);  h = mul(inv_projection_view,
 *              (NDC, 1)) row by row as in oxc_decode_visbuffer;  world = h.xyz / h.w, three divisions.
 *   4. frame   (:63-67)  V = normalize(camera_position - world);  N = normalize(mapped) (a second normalisation, as the Slang);  R =
 *              reflect(-V, N);  NoV = |dot(N, V)| + 1e-5f;  NoL = max(dot(N, L), 0.0), L = sun_dir as given (not normalised).
 *   5. sky     (:69-71)  With OXC_SCENE_HAS_SKY and depth == 0.0 the colour is sky_has_texture != 0 ? (1, 1, 1) : sky_solid_color.rgb and the
 *              pixel is done (class "sky"; it cannot be reached with a transparent background, so its alpha is never stored).  Without
 *              either flag a pixel with depth == 0.0 runs on as the Slang does (class "fall-through empty"): the IEEE results are the rule,
 *              a division by a zero h.w included.
 *   6. terms   (:73-84)  directional_shadow = HasDirectionalLight ? resolved_shadows texel : 1.0;  contact_shadow = HasContactShadows ?
 *              contact_shadows texel : 1.0;  visibility = directional_shadow * contact_shadow;  direct = HasDirectionalLight ? sun_intensity
 *              : 0.0;  env = HasSky ? sky_ambient_color : base_ambient_color.  An image whose flag is clear is not read.
 *   7. surface (pbr.slang:6-9, 35-50, 69-73; hoisted: BRDF recomputes them with the same operands for every light)  F0 = lerp(0.04f, albedo,
 *              metallic) per channel;  alpha = max(roughness * roughness, 0.0025f);  alpha2 = alpha * alpha;
 *              GGX_directional_albedo(NoV, alpha): x = NoV, y = alpha, x2 = x * x, y2 = y * y;  per component k of the nine float4 constants
 *              c0..c8 as the Slang lists them:  r_k = (((((((c0 + c1 * x) + c2 * y) + (c3 * x) * y) + c4 * x2) + c5 * y2) + (c6 * x2) * y) +
 *              (c7 * x) * y2) + (c8 * x2) * y2;  AB = (clamp(r_0 / r_2, 0.0, 1.0), clamp(r_1 / r_3, 0.0, 1.0));  Ess = saturate(AB.x + AB.y);
 *              energy_compensation = 1.0 + (F0 * (1.0 - Ess)) / max(Ess, 1e-4f) per channel.
 *   8. ambient (:86-100)  kS = F0 * AB.x + AB.y;  kD = (1.0 - metallic) * (1.0 - kS);  spec_occlusion = saturate((pow(NoV + occlusion,
 *              exp2(-16.0 * roughness - 1.0)) - 1.0) + occlusion), pow the pow rule (a base below 2^-126, negative or NaN gives 0), exp2 the
 *              exp2 rule below;  ibl_diffuse = ((kD * env) * albedo) * Fd_Lambert();  ibl_specular = (kS * env) * spec_occlusion;  indirect =
 *              ibl_diffuse * occlusion + ibl_specular.
 *   9. lights  (:102-113, pbr.slang:89-172)  total = 0;  for i = 0 .. light_count - 1 in order, light = lights[i] (64 bytes: position f32x3,
 *              intensity, color f32x3, range, direction f32x3, inner_cone_angle, outer_cone_angle, kind u32, two pad words).  kind == 1
 *              (Point) and kind == 2 (Spot) are shaded; every other value (0 = Directional included) is skipped, as the Slang's if / else if.
 *              lv = light.position - world;  dist = length(lv);  Ll = lv / dist;  attenuation = lights_attenuate_point(dist, range): range <=
 *              0.0 gives 1.0 / (dist * dist + 0.1f);  otherwise (a NaN range too) win = dist / range, win = ((win * win) * win) * win, win =
 *              max(0.0, 1.0 - win), win = win * win, win / (dist * dist + 0.1f).  Spot: attenuation = attenuation * smoothstep(cos(outer),
 *              cos(inner), dot(-Ll, normalize(direction))), cos the cos rule below.  attenuation <= 0.0 || intensity <= 0.0 ends the light
 *              (outcome "attenuation or intensity out"; a NaN passes both tests);  NdotL = saturate(dot(N, Ll));  NdotL <= 0.0 ends it
 *              (outcome "NdotL out").  Otherwise (outcome "shaded") b = BRDF(V, N, Ll) of step 10;  radiance = (color * attenuation) *
 *              intensity;  total += ((b.diffuse + b.specular) * radiance) * NdotL per channel.  A light that ends early adds nothing.
 *  10. BRDF(V, N, l)  (pbr.slang:11-24, 61-87)  VL = V + l;  H = dot(VL, VL) > 1e-8f ? normalize(VL) : N;  NoLb = saturate(dot(N, l));  NoH =
 *              saturate(dot(N, H));  LoH = saturate(dot(l, H));  f = (NoH * alpha2 - NoH) * NoH + 1.0;  D = alpha2 / ((PI * f) * f + 1e-7f);
 *              GGXV = NoLb * sqrt((NoV * NoV) * (1.0 - alpha2) + alpha2);  GGXL = NoV * sqrt((NoLb * NoLb) * (1.0 - alpha2) + alpha2);  Vis =
 *              saturate(0.5 / ((GGXV + GGXL) + 1e-7f));  F = F0 + (1.0 - F0) * pow(saturate(1.0 - LoH), 5.0) per channel, the pow rule;
 *              specular = ((D * Vis) * F) * energy_compensation;  diffuse = (((1.0 - metallic) * (1.0 - F)) * albedo) * Fd_Lambert().
 *  11. sun     (:115-123)  horizon = saturate(1.0 + 1.3f * dot(R, smooth));  horizon = horizon * horizon;  surface = 0;  if NoL > 0.0 (class
 *              "lit, NoL > 0"; otherwise "lit, NoL == 0"):  b = BRDF(V, N, L);  surface = (((b.diffuse + b.specular * horizon) * direct) *
 *              NoL) * visibility per channel.
 *  12. store   (:125-126)  colour = ((surface + total) + indirect) + emission per channel, alpha = 1.0.  Without
 *              OXC_SCENE_TRANSPARENT_BACKGROUND final_attachment is B10G11R11 UfloatPack32: R, G, B packed as UF11, UF11, UF10 by the rule of
 *              oxc_decode_visbuffer step 8.  With it, R16G16B16A16 Sfloat: each channel converted to binary16 with round to nearest even,
 *              denormals kept, a NaN stored as 0x7E00 (oxc_decode_visbuffer step 5), R in the lowest half.  So no NaN bit pattern of the
 *              arithmetic reaches the image.
 * exp2 rule, for a binary32 t:  y = (double)t, then the second half of the pow rule: k = floor(y + 0.5), r = y - k, E(r * ln 2) * 2^k rounded
 *   to binary32 once; y <= -160 gives 0.0, y >= 160 gives +Inf, NaN gives NaN.
 * cos rule, for a binary32 x:  a non-finite x or |x| > 2^24 gives NaN (so a spot light with such an angle ends at its attenuation test).
 *   Otherwise in binary64, no contraction:  a = |x|;  q = floor(a * 0x1.45f306dc9c883p-1 + 0.5) (an integer below 2^24);  r = (a - q *
 *   0x1.921fb54p+0) - q * 0x1.10b4611a62633p-30 (pi / 2 in two constants: the first has 29 significant bits, so its product with q is
 *   exact);  z = r * r;  S = r + (r * z) * ps(z), Cc = 1.0 + z * pc(z) with the two polynomials of the rotation rule of oxc_resolve_shadowmap
 *   step 6;  cos = Cc, -S, -Cc, S for q mod 4 = 0, 1, 2, 3, rounded to binary32 once.  Within one binary32 ulp of the correctly rounded
 *   cosine on [0, pi] (tests/test_pbr_apply_model.py).
 * Limits (else OXC_INVALID_ARG, nothing launched, the output untouched): width and height not zero, at most 65536 a side and equal to the
 * depth attachment's; depth_attachment one R32F level at offset 0; albedo, emissive and metallic_roughness_occlusion 4-byte aligned with one
 * u32 per pixel; normal_attachment 8-byte aligned with one u16x4 per pixel; ambient_occlusion_attachment 2-byte aligned with one u16 per
 * pixel; resolved_shadows_attachment (read with HasDirectionalLight) and contact_shadows_attachment (read with HasContactShadows) one R32F
 * level of the depth's extent at offset 0 -- an image whose flag is clear is not read, not checked and may be null; lights_buffer 4-byte
 * aligned with light_count records of 64 bytes (may be null when light_count is 0); final_attachment 4-byte aligned with one u32 per pixel,
 * or 8-byte aligned with one u16x4 per pixel with a transparent background; every host scalar (the matrix, camera_position, sun_dir,
 * sun_intensity, the three colours) finite.  Light records live on the device and are not validated: the rule gives a defined result for
 * any bit pattern in them.  One launch, no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
#define OXC_SCENE_HAS_DIRECTIONAL_LIGHT (1u << 0)  /* GPU::SceneFlags (scene.slang:242-256); the other bits are not read */
#define OXC_SCENE_HAS_ATMOSPHERE (1u << 1)         /* oxc_apply_pbr: OXC_INVALID_ARG; the branch is oxc_apply_pbr_atmosphere */
#define OXC_SCENE_HAS_CONTACT_SHADOWS (1u << 9)
#define OXC_SCENE_HAS_SKY (1u << 10)
#define OXC_SCENE_TRANSPARENT_BACKGROUND (1u << 11)
typedef struct oxc_pbr_context {
  uint32_t struct_size; /* sizeof(oxc_pbr_context) */
  uint32_t width, height;
  uint32_t scene_flags;           /* GPU::SceneFlags */
  uint32_t light_count;
  uint32_t sky_has_texture;       /* GPU::Sky::has_texture */
  float inv_projection_view[16];  /* Camera::inv_projection_view, column-major */
  float camera_position[3];
  float sun_dir[3];               /* L: towards the sun, used as given */
  float sun_intensity;            /* Li */
  float base_ambient_color[3];    /* the engine passes 0.03 */
  float sky_solid_color[4];       /* GPU::Sky::solid_color */
  float sky_ambient_color[3];     /* GPU::Sky::ambient_color */
  oxc_image depth_attachment;     /* in: R32F, levels = 1, reversed Z */
  oxc_buffer albedo_attachment;   /* in: R8G8B8A8 sRGB, u32[height][width], R in the low byte */
  oxc_buffer normal_attachment;   /* in: u16x4[height][width], .rg mapped, .ba smooth */
  oxc_buffer emissive_attachment; /* in: B10G11R11 UfloatPack32, u32[height][width] */
  oxc_buffer metallic_roughness_occlusion_attachment; /* in: R8G8B8A8 Unorm, u32[height][width] */
  oxc_buffer ambient_occlusion_attachment;            /* in: binary16 as u16[height][width] */
  oxc_image resolved_shadows_attachment;              /* in: R32F, read with HasDirectionalLight */
  oxc_image contact_shadows_attachment;               /* in: R32F, read with HasContactShadows */
  oxc_buffer lights_buffer;       /* in: GPU::Light[light_count], 64 bytes each (scene.slang:272-283) */
  oxc_buffer final_attachment;    /* out: u32[height][width] B10G11R11, or u16x4[height][width] with a transparent background */
} oxc_pbr_context;

oxc_status oxc_apply_pbr(oxc_ctx* ctx, const oxc_pbr_context* context, void* hip_stream);

/* ---- eye adaptation: the luminance histogram of the lit HDR image and the exposure it gives ---------------------------------
 * Replaces RendererInstance::apply_eye_adaptation (Oxylus/src/Render/Passes/PostProcess.cpp:7-77, pipelines histogram_generate and
 * histogram_average, passes/histogram_generate.slang, passes/histogram_average.slang, passes/histogram.slang, com::remap at
 * common/math.slang:203), the pass directly behind apply_pbr and the first reader of its image: a 256-bin log-luminance histogram of
 * final_attachment, reduced to GPU::HistogramLuminance {adapted_luminance, exposure}, the record bloom_prefilter and tonemap multiply by.
 * Out of scope: bloom, tone mapping and the lens effects, the atmosphere branch, any change to what oxc_apply_pbr writes.
 * time_coeff is taken as given: the reference computes 1 - glm::exp(-adaptation_speed * delta_time) on the host with the platform's exp,
 * which no checker can pin, so it stays outside the parity claim; the C++ shim and the Python twin compute it from adaptation_speed and
 * delta_time with their own expf and pass the result on.
 * Arithmetic: the canonical binary32 arithmetic of oxc_apply_pbr -- round to nearest even, left to right, no contraction, IEEE division
 * (1.0 / x is a division), max through fmaxf, a comparison with a NaN operand is false; a float to int conversion truncates and saturates
 * and gives 0 for a NaN.  log2 is the log2 rule of oxc_generate_ambient_occlusion (rounded to binary32 once; NaN and everything below
 * 2^-126 give -Inf, +Inf gives +Inf), exp2 the exp2 rule of oxc_apply_pbr.  The checker is tests/eye_adaptation_model.py.
 * Per pixel (x, y) of the W x H image (histogram_generate.slang:19-43):
 *   1. decode    (:35)  Stated rule, as for the albedo tap of oxc_apply_pbr: the Slang's Load is a load of texel (x, y).  source_format 0:
 *              R = UF11 of bits 0-10, G = UF11 of bits 11-21, B = UF10 of bits 22-31 by the exact decode of oxc_apply_pbr step 2 (exponent
 *              field 31 is +Inf for a zero mantissa, NaN otherwise).  source_format 1: halves 0, 1, 2 through binary16 -> binary32, exact,
 *              denormals kept; alpha is not read.
 *   2. luminance (:36)  luminance = (r * 0.2127f + g * 0.7152f) + b * 0.0722f, the constants as the Slang writes them.
 *   3. dark      (:20-22)  luminance < 0.001f gives bin 0 (a negative or -0 luminance from RGBA16F too); a NaN fails the test and goes on.
 *   4. bin       (:24-25)  l = log2(luminance);  mapped = ((l - min_exposure) / (max_exposure - min_exposure)) * 254.0f + 1.0f (com::remap
 *              with the output range 1 .. 255; the difference of the two exposures is one binary32 subtraction);  bin = clamp(i32(mapped),
 *              0, 255).  So a NaN luminance gives bin 0 and +Inf gives bin 255.
 *   5. count     (:38-42)  histogram[bin] += 1.  The counts are integers: the result does not depend on the order.
 * Once per call (histogram_average.slang:22-50):
 *   6. weighted sum (:36-43)  weighted_sum = sum over k of histogram[k] * k in u32, modulo 2^32 as the Slang's InterlockedAdd gives it;
 *              dark = f32(histogram[0]);  pixel_count = f32(width * height);  avg = f32(weighted_sum) / max(pixel_count - dark, 1.0f) - 1.0f.
 *   7. desired   (:44)  desired = exp2(((avg / 254.0f) * (max_exposure - min_exposure)) + min_exposure).
 *   8. adaptation (:45-46)  last = exposure_buffer.adapted_luminance;  adapted = last + (desired - last) * time_coeff.
 *   9. exposure  (:22-26, :47-49)  ev100 = log2(adapted * ((100.0f * ev100_bias) / 12.5f));  exposure = 1.0f / (exp2(ev100) * 1.2f);  store
 *              {adapted, exposure}.  A NaN in either word is stored as 0x7FC00000: no NaN bit pattern of the arithmetic reaches memory.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written): width and height not zero and at most 65536 a side, width * height at
 * most 2^32 - 1; source_format 0 or 1; final_attachment 4-byte aligned with one u32 per pixel (format 0) or 8-byte aligned with one u16x4
 * per pixel (format 1); histogram_buffer 4-byte aligned, 1024 bytes; exposure_buffer 4-byte aligned, 8 bytes; min_exposure, max_exposure,
 * ev100_bias, time_coeff and max_exposure - min_exposure finite; max_exposure > min_exposure.  The exposure buffer's content is device
 * data and is not validated: the rule is defined for any bit pattern in it.  histogram_buffer stands for the reference's transient
 * histogram_bin_indices_buffer; after the call it holds this frame's counts.  exposure_buffer is caller-owned and persists between frames;
 * the caller initialises it to {1.0f, 1.0f}, as RendererInstance.cpp:1778-1784 fills it.  The histogram is zeroed in-stream by a kernel;
 * three launches, no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
#define OXC_SCENE_HAS_EYE_ADAPTATION (1u << 2) /* GPU::SceneFlags (RendererInstance.cpp:1278); oxc_apply_eye_adaptation does not read it, oxc_apply_bloom's scene_flags does */
typedef struct oxc_eye_adaptation_context {
  uint32_t struct_size; /* sizeof(oxc_eye_adaptation_context) */
  uint32_t width, height;
  uint32_t source_format;       /* 0: B10G11R11 UfloatPack32, u32[height][width];  1: R16G16B16A16 Sfloat, u16x4[height][width] */
  float min_exposure;           /* GPU::HistogramLuminanceInfo: -6 (the component: -11.5) */
  float max_exposure;           /* 18 */
  float ev100_bias;             /* 1 */
  float time_coeff;             /* 1 - exp(-adaptation_speed * delta_time), computed by the caller */
  oxc_buffer final_attachment;  /* in: what oxc_apply_pbr wrote */
  oxc_buffer histogram_buffer;  /* out: u32[256] */
  oxc_buffer exposure_buffer;   /* in/out: {f32 adapted_luminance, f32 exposure} */
} oxc_eye_adaptation_context;

oxc_status oxc_apply_eye_adaptation(oxc_ctx* ctx, const oxc_eye_adaptation_context* context, void* hip_stream);

/* ---- bloom: the prefiltered half-resolution image, its downsample pyramid and the upsample pyramid the tonemap reads -------------
 * Replaces RendererInstance::apply_bloom (Oxylus/src/Render/Passes/PostProcess.cpp:79-203, pipelines bloom_prefilter, bloom_downsample
 * and bloom_upsample: passes/bloom_prefilter.slang, passes/bloom_downsample.slang, passes/bloom_upsample.slang, com::luminance at
 * common/color.slang:79-81, the extents at RendererInstance.cpp:509-510 and 1257-1267, Texture::calculate_mip_count at
 * include/Asset/Texture.hpp:144-146, the samplers LinearSamplerBorder and LinearSamplerClamped at include/Render/Utils/VukCommon.hpp:
 * 103-120), the pass directly behind apply_eye_adaptation and the first reader of its exposure.
 * Out of scope: the atmosphere branch.  bloom_intensity is set by apply_bloom for the tonemap: the C++ shim and the Python twin
 * carry it to oxc_apply_tonemap, this call does not read it.
 * Arithmetic: the canonical binary32 arithmetic of oxc_apply_pbr -- round to nearest even, left to right, no contraction, IEEE division
 * (1.0 / x is a division), min / max through fminf / fmaxf (a NaN operand gives the other one), clamp(x, a, b) = min(max(x, a), b),
 * lerp(a, b, t) = a + (b - a) * t.  UF11 / UF10 decode is the exact decode of oxc_apply_pbr step 2, the pack the truncating one of
 * oxc_decode_visbuffer step 8 (a NaN becomes the one fixed pattern, negatives become 0); binary16 conversion as in oxc_apply_pbr step 12
 * (round to nearest even, denormals kept, a NaN stored as 0x7E00; binary16 -> binary32 exact).  The checker is tests/bloom_model.py.
 * Geometry: the source is W x H; the bloom extent is (w2, h2) = (W / 2, H / 2), integer divisions; L = floor(log2(max(w2, h2))) + 1
 * levels, computed in integers -- equal to the reference's u32(log2f(f32(m))) + 1 for every side the limits allow (m < 8192 is exact in
 * binary32, and a correctly rounded log2f of such an m is below the next integer unless m is that power of two); level k is
 * max(1, w2 >> k) x max(1, h2 >> k); two pyramids of that shape, bloom_downsampled (D) and bloom_upsampled (U).  Level L - 1 is 1 x 1.
 * Sampling (stated difference, as in oxc_contact_shadows step 6 and oxc_generate_ambient_occlusion step 9): a hardware linear sampler
 * has fixed-point weights of an implementation-defined width, so the rule is the manual bilinear.  For the output pixel (x, y) of an
 * ow x oh output reading an sw x sh source level with the tap offset (kx, ky):  uv = ((f32(x) + 0.5) / f32(ow), (f32(y) + 0.5) / f32(oh));
 * ts = (1.0 / f32(ow), 1.0 / f32(oh)) -- from the OUTPUT extent, as the shaders write it;  p = uv + ts * (kx, ky);
 * g = p * (f32(sw), f32(sh)) - 0.5;  i = floor(g) converted to i32 saturating;  f = g - floor(g);  the four texels are
 * (i.x + {0, 1}, i.y + {0, 1});  the result is lerp(lerp(t00, t10, f.x), lerp(t01, t11, f.x), f.y) per channel.  Address modes:
 * border (LinearSamplerBorder, transparent black): a texel whose x or y lies outside [0, size - 1] is (0, 0, 0) -- not clamped;
 * clamp (LinearSamplerClamped): each coordinate is clamped to [0, size - 1], exactly as oxc_contact_shadows does.
 * The tap offsets (bloom_prefilter.slang:51-63, bloom_downsample.slang:21-33): a (-2, 2), b (0, 2), c (2, 2), d (-2, 0), e (0, 0),
 * f (2, 0), g (-2, -2), h (0, -2), i (2, -2), j (-1, 1), k (1, 1), l (-1, -1), m (1, -1);  of the upsample (bloom_upsample.slang:31-39):
 * a (-1, 1), b (0, 1), c (1, 1), d (-1, 0), e (0, 0), f (1, 0), g (-1, -1), h (0, -1), i (1, -1).
 *   1. clear     (RendererInstance.cpp:1267, PostProcess.cpp:98)  The texel of level L - 1 of U is stored as zero (alpha 1.0 with RGBA16F,
 *              step 5).  The reference clears both pyramids to black; every other level of both is fully overwritten below, so after the
 *              call every byte of both pyramids is defined.  With L = 1 that level is U's level 0: the bloom the tonemap reads is black.
 *              The clear is done by a kernel in-stream.
 *   2. prefilter (bloom_prefilter.slang:41-87)  Output D level 0, source the W x H final image, border.  The 13 taps a..m.
 *              exposure = OXC_SCENE_HAS_EYE_ADAPTATION ? the second word of exposure_buffer : 1.0 -- device data, any bit pattern.
 *              Five groups per channel: (((a + b) + d) + e) * 0.25 * exposure, (((b + c) + e) + f) ..., (((d + e) + g) + h) ...,
 *              (((e + f) + h) + i) ..., (((j + k) + l) + m) ... .  Then in that order over the groups: group = min(group, clamp_value)
 *              per channel;  weight = 1.0 / (1.0 + ((r * 0.299f + g * 0.587f) + b * 0.114f));  prefilter(group): brightness = max(r,
 *              max(g, b)), knee = threshold * soft_threshold, soft = clamp((brightness - threshold) + knee, 0.0, 2.0 * knee),
 *              soft = ((soft * soft) * 0.25) / (knee + 1.0e-5f), contribution = max(soft, brightness - threshold) / max(brightness,
 *              1.0e-5f), group * contribution per channel;  color_sum += prefilter(group) * weight (from 0.0);  weight_sum += weight
 *              (from 0.0).  Store color_sum / (weight_sum + 1.0e-5f) per channel.
 *   3. downsample (bloom_downsample.slang:12-40, PostProcess.cpp:136-163)  For k = 1 .. L - 1 in order: output D level k, source D level
 *              k - 1, border, the 13 taps:  result = ((((a + c) + g) + i) * 0.03125 + (((b + d) + f) + h) * 0.0625) + ((((e + j) + k) + l)
 *              + m) * 0.125.
 *   4. upsample  (bloom_upsample.slang:18-47, PostProcess.cpp:169-202)  For k = L - 1 down to 1 in order: output U level k - 1; the 9-tap
 *              source is D level L - 1 when k = L - 1, else U level k; clamp.  color_sum = (e * 0.25 + (((b + d) + f) + h) * 0.125) +
 *              (((a + c) + g) + i) * 0.0625.  source_color: the Slang's un-offset SampleLevel of D level k - 1 samples a level of the
 *              output's own extent at the pixel centre; the stated rule, as for the albedo tap of oxc_apply_pbr, is a load of texel (x, y).
 *              Store lerp(source_color, color_sum, radius).
 *   5. formats   source_format 0: the source and both pyramids are B10G11R11 UfloatPack32, one u32 per texel.  source_format 1
 *              (transparent background): R16G16B16A16 Sfloat, one u16x4 per texel; alpha is never read and is stored as 1.0 (0x3C00).
 *              A decision the reference leaves open: its shaders declare the storage images R11F_G11F_B10F while same_format_as(
 *              final_attachment) makes them RGBA16F in that mode, and no Vulkan rule defines what such a store does; the rule here is
 *              the attachment's format.  Every level is packed when stored and decoded when the next step reads it: the truncation of
 *              the pack is part of the result.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message): width and
 * height at least 2 and max(width, height) / 2 < 8192 (so L <= 13); source_format 0 or 1; final_attachment aligned to its texel (4 or 8
 * bytes) with one texel per pixel; both pyramids with width == W / 2, height == H / 2, levels == L; every level aligned to its texel and
 * inside the pyramid's `bytes`; the levels of a pyramid do not overlap each other; no level of one pyramid shares a byte with a level of the other or
 * with the source; exposure_buffer, when read, 4-byte aligned and 8 bytes (without the flag it is not looked at and may be null);
 * threshold, soft_threshold, clamp_value and radius finite.  No scratch, no allocation, no host synchronisation; capturable into a HIP
 * graph on one stream as a linear chain of kernels. */
#define OXC_SCENE_HAS_BLOOM (1u << 3) /* GPU::SceneFlags (RendererInstance.cpp:1282); oxc_apply_bloom does not read it, oxc_apply_tonemap's scene_flags does */
/* A mip pyramid of 4-byte (B10G11R11) or 8-byte (R16G16B16A16 Sfloat) texels in one device allocation: oxc_image's fields under the
 * same names, then the allocation's size.  Level k is max(1, width >> k) x max(1, height >> k) texels, row-major, at byte offset
 * level_offset[k]; the levels may lie in any order and with gaps. */
typedef struct oxc_image_pyramid {
  void* dptr;
  uint32_t width, height, levels, _pad;
  uint64_t level_offset[13];
  uint64_t bytes;
} oxc_image_pyramid;
typedef struct oxc_bloom_context {
  uint32_t struct_size; /* sizeof(oxc_bloom_context) */
  uint32_t width, height;
  uint32_t source_format;       /* 0: B10G11R11 UfloatPack32;  1: R16G16B16A16 Sfloat -- the source and both pyramids */
  uint32_t scene_flags;         /* only OXC_SCENE_HAS_EYE_ADAPTATION is read */
  float threshold;              /* pp.bloom_threshold: 1.0 (RendererCVar.cpp:44-48) */
  float soft_threshold;         /* 0.125 */
  float clamp_value;            /* 4.0 */
  float radius;                 /* 0.75 */
  uint32_t _pad;
  oxc_buffer final_attachment;  /* in: what oxc_apply_pbr wrote */
  oxc_buffer exposure_buffer;   /* in, read only with OXC_SCENE_HAS_EYE_ADAPTATION: {f32 adapted_luminance, f32 exposure} */
  oxc_image_pyramid bloom_downsampled_attachment; /* out: D */
  oxc_image_pyramid bloom_upsampled_attachment;   /* out: U; level 0 is what the tonemap reads */
} oxc_bloom_context;

oxc_status oxc_apply_bloom(oxc_ctx* ctx, const oxc_bloom_context* context, void* hip_stream);

/* ---- tonemap: exposure, bloom composite, tone curve, lens effects and the 8-bit image ------------------------------------------
 * Replaces RendererInstance::apply_tonemap (Oxylus/src/Render/Passes/PostProcess.cpp:205-247, pipeline tonemap: passes/tonemap.slang,
 * passes/lens.slang, common/color.slang:4-55, GPU::PostProcessSettings and GPU::TonemapType at include/Scene/SceneGPU.hpp:295-309, the
 * scene flags at SceneGPU.hpp:258-266, the swapchain formats at RenderContext.cpp:102-105), the last pass of the frame: the HDR image
 * oxc_apply_pbr wrote, times the exposure oxc_apply_eye_adaptation left behind, plus level 0 of the upsample pyramid oxc_apply_bloom wrote,
 * through one of four tone curves and three lens effects into one 8-bit word per pixel.
 * Out of scope: the atmosphere branch (FXAA, which the reference runs on the HDR image before the eye adaptation, is oxc_apply_fxaa), the unused
 * agx_tonemapping (tonemap.slang:90-129) and the Jzazbz UCS (TONE_MAPPING_UCS is ICtCp).
 * Arithmetic: the canonical binary32 arithmetic as the oxc_apply_bloom block states it (round to nearest even, left to right, no
 * contraction, IEEE division and square root, min / max through fminf / fmaxf, clamp, lerp, the UF11 / UF10 / binary16 decodes), a
 * comparison with a NaN operand is false, a float to int conversion truncates, saturates and gives 0 for a NaN; mul(M, v) row r is
 * (M[r][0] * v.x + M[r][1] * v.y) + M[r][2] * v.z and mul(A, B) element (r, c) is (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c];
 * dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; a decimal literal is the binary32 nearest to it.  The checker is tests/tonemap_model.py.
 * Per pixel (x, y) of the W x H image (tonemap.slang:668-723), in this order:
 *   1. source    (:670-671)  Stated rule, as in oxc_apply_bloom step 4: SampleLevel(input_image, tex_coord) of an image of the output's own
 *              extent at the pixel centre is a load of texel (x, y).  source_format 0: the exact UF11 / UF11 / UF10 decode, alpha 1.0;
 *              source_format 1: four halves through binary16 -> binary32, exact, denormals kept; alpha is the fourth.
 *   2. exposure  (:673-678)  OXC_SCENE_HAS_EYE_ADAPTATION: color *= the second word of exposure_buffer (device data, any bit pattern);
 *              else color *= exposure (post_process_settings.exposure).
 *   3. bloom     (:680-683)  OXC_SCENE_HAS_BLOOM: color += bloom * bloom_intensity per channel (the product rounded, then the sum), bloom the
 *              manual bilinear of the oxc_apply_bloom block on level 0 of bloom_upsampled_attachment, (W / 2) x (H / 2), at uv = ((f32(x) +
 *              0.5) / f32(W), (f32(y) + 0.5) / f32(H)): g = uv * (f32(sw), f32(sh)) - 0.5, i = floor(g) converted to i32 saturating,
 *              f = g - floor(g), lerp(lerp(t00, t10, f.x), lerp(t01, t11, f.x), f.y).  The stated difference about hardware samplers is the
 *              same.  Address mode: repeat -- the texel coordinates are i0 = floor_mod_i(i, size) and i1 = (i0 + 1 == size ? 0 : i0 + 1)
 *              per axis, both in [0, size - 1] for every bit pattern of uv.  STATED ASSUMPTION: the pass binds a sampler created with
 *              only its filters set (PostProcess.cpp:228), and a zero-initialised VkSamplerCreateInfo has address mode repeat; vuk's
 *              SamplerCreateInfo defaults could not be read where this was written.  tools/reference_capture/ is where a capture of the
 *              reference would pin it.
 *   4. tone curve by tonemap_type (:685-702):
 *              0 None   nothing is applied (no clamp either: the store saturates).
 *              1 ACES   ACES_Fitted (:37-69): v = mul(ACESInputMat, color); per channel a = v * (v + 0.0245786f) - 0.000090537f,
 *                       b = v * (0.983729f * v + 0.4329510f) + 0.238081f, a / b; mul(ACESOutputMat, .); saturate.
 *              2 AgX    AgX_DS (:131-262): w = max(color, 0.0); w = mul(sRGB_to_adjusted, w); per channel color_DualSection(x, 0.10, 1.0):
 *                       x < S ? x : peak - (peak - S) * exp((-C * (x - S)) / peak) with S = peak * linear, C = peak / (peak - S); clamp 0..1;
 *                       d = dot(w, (0.2126729, 0.7151522, 0.0721750)); w = clamp(d + (w - d) * 1.3, 0, 1); mul(inverse(sRGB_to_adjusted), w).
 *              3 GT7    (:267-666) rec2020 = mul(XYZ_TO_REC2020_MAT, mul(REC709_TO_XYZ_MAT, color)) (two products, as written); GT7ToneMapping
 *                       initializeAsSDR + applyToneMapping with the ICtCp UCS: rgbToICtCp and iCtCpToRgb with every sum left to right as
 *                       written ((r * 1688.0f + g * 2146.0f) + b * 262.0f) / 4096.0f ...), inverseEotfSt2084 = exp2(m2 * (log2(c1 + c2 * ym) -
 *                       log2(1.0f + c3 * ym))) with ym = pow(v * 100.0f / 10000.0f, m1), eotfSt2084 with its three clamps as ifs (a NaN
 *                       passes them), evaluateCurve: x < 0 gives 0; x < linearSection_ * peakIntensity_ gives weightToe * (midPoint_ *
 *                       pow(x / midPoint_, toeStrength_)) + weightLinear * x; else kA_ + kB_ * exp(x * kC_); smoothStep(x, e0, e1): t =
 *                       (x - e0) / (e1 - e0), x < e0 gives 0, x > e1 gives 1, else (t * t) * (3.0f - 2.0f * t); out = sdrCorrectionFactor_ *
 *                       min((1.0f - blendRatio_) * skewed + blendRatio_ * scaled, framebufferLuminanceTarget_); then
 *                       mul(XYZ_TO_REC709_MAT, mul(REC2020_TO_XYZ_MAT, out)).  pow(y, m1) of a negative Rec.2020 channel (a saturated
 *                       Rec.709 colour has one) is 0 by rule 6, where the reference's pow is undefined.
 *   5. constants  Everything of 4 and 7 that does not depend on the pixel is evaluated ONCE per call, in the canonical binary32, in the order
 *              the Slang writes it, ON THE HOST (the library's host code is compiled without contraction and uses the rule functions of 6,
 *              not the platform's libm) and reaches the kernel as arguments: color_PrimariesToMatrix / color_ComputeCompressionMatrix /
 *              inverse (:131-202) for sRGB_to_XYZ, adjusted_to_XYZ, XYZ_to_adjusted, sRGB_to_adjusted = mul(sRGB_to_XYZ, XYZ_to_adjusted)
 *              and inverse(sRGB_to_adjusted); S, peak - S and -C of color_DualSection; kA_, kB_, kC_ (kB_ = ((-peak) * k) * exp(
 *              linearSection_ / k)), linearSection_ * peakIntensity_, framebufferLuminanceTarget_ = 250.0f / 100.0f,
 *              framebufferLuminanceTargetUcs_ = rgbToICtCp((target, target, target))[0], sdrCorrectionFactor_ = 1.0f / (250.0f / 100.0f),
 *              1.0f - blendRatio_, the two e1 - e0, m2 = 78.84375f * 1.0f, 1.0f / m2, 1.0f / m1; FfxLensGetRGMag.  The checker evaluates
 *              them the same way.
 *   6. transcendentals  (stated difference: the reference's are implementation-defined)  pow(v, p) is the pow rule of oxc_apply_pbr,
 *              exp2((double)p * L(v)) rounded once, and L of a negative, zero, denormal or NaN v is -Inf: such a base gives 0 for p > 0.
 *              log2 is the log2 rule rounded to binary32 once; exp2 the exp2 rule; exp(x) = the exp2 rule's binary64 half of
 *              (double)x * 0x1.71547652b82fep+0, rounded once; sqrt is IEEE.  cos(a): a non-finite a gives NaN; otherwise
 *              u = (double)|a| * 0x1.45f306dc9c883p-3, t = (float)(u - floor(u)), t == 1.0f becomes 0, and the result is the cosine of the
 *              rotation rule of oxc_resolve_shadowmap step 6 at the turn t.
 *   7. chromatic aberration (:704-707, lens.slang:51-88)  OXC_SCENE_HAS_CHROMATIC_ABERRATION.  AS THE REFERENCE WRITES IT, the three channels
 *              are re-sampled from the UN-EXPOSED, UN-TONEMAPPED input_image and REPLACE color: steps 2-4 have no effect on the pixel then.
 *              That is kept.  center = (W / 2, H / 2), integer divisions; rcp = 1.0f / f32(2 * center) per axis; (redMag, greenMag) =
 *              FfxLensGetRGMag(chromatic_aberration_amount): B = 0.00459f * amount, n(w) = 1.5220f + B / (w * w) for w = 0.612f, 0.549f,
 *              0.464f, redMag = (n_r - 1.0f) / (n_b - 1.0f), greenMag likewise.  redShift = ((f32(coord - center) * redMag + f32(center)) +
 *              0.5f) * rcp, greenShift with greenMag, blue at f32(coord) * rcp (no half, as written).  red = .r of the manual bilinear of
 *              the W x H source at redShift with the repeat rule of 3, green = .g at greenShift, blue = .b.  W or H of 1 makes rcp(0)
 *              infinite: the canonical arithmetic defines the result (Inf and NaN coordinates convert saturating, the weights are NaN,
 *              the channel is NaN and stores as 0).  No special case.
 *   8. vignette  (:709-711, lens.slang:115-125)  OXC_SCENE_HAS_VIGNETTE.  per axis m = cos(((f32(|coord - center|) / f32(center)) *
 *              vignette_amount) * piOver4), piOver4 = 3.1415926535897932384626433832795f * 0.25f; m = m * m; m = m * m; color *=
 *              clamp(m.x * m.y, 0, 1), and clamp of a NaN is 0.  A centre of 0 gives 0 / 0 = NaN: the pixel becomes 0.
 *   9. film grain (:713-719, lens.slang:9-44, 98-106)  OXC_SCENE_HAS_FILM_GRAIN.  v = pcg3d16(u32x3(coord / divisor, film_grain_seed)) in
 *              wrapping u32; fine = f32(v.xy) * (1.0 / 65536.0) - 0.5, exact; P = f32(coord) / film_grain_scale + fine; simplex(P): u =
 *              (P.x + P.y) * F2, Pi = round(P + u) with halves to even (SPIR-V leaves halves open; stated), v = (Pi.x + Pi.y) * G2,
 *              Pf0 = P - (Pi - v), F2 and G2 the binary32 nearest (sqrt(3) - 1) / 2 and (3 - sqrt(3)) / 6; grain = 1.0f - 2.0f *
 *              exp2((-sqrt(Pf0.x * Pf0.x + Pf0.y * Pf0.y)) * 3.0f); color = color + (grain * min(color, 1.0f - color)) * film_grain_amount.
 *              A decision the reference leaves open: coord / (i32)(grainScaleVal / 8) divides by zero for every scale below 8, the
 *              engine's default 1.0 included (the FidelityFX original divides in floating point).  The rule here: divisor = the saturating
 *              truncation of film_grain_scale / 8.0f, and a divisor of 0 is taken as 1; a negative one is refused by the limits.
 *  10. alpha     (:721)  OXC_SCENE_TRANSPARENT_BACKGROUND ? the source's alpha : 1.0.
 *  11. store     output_format 0: R8G8B8A8 Srgb, 1: B8G8R8A8 Srgb (the swapchain formats), 2: R8G8B8A8 Unorm; byte 0 is the first-named
 *              channel.  Srgb formats, per colour channel: c = saturate(color); c <= 0.0031308f ? c * 12.92f : 1.055f * pow(c, p) - 0.055f
 *              with p the binary32 nearest 1 / 2.4; then u32(floor(saturate(e) * 255.0f + 0.5f)) as in oxc_decode_visbuffer.  Alpha and
 *              format 2 go through that last expression directly.  A NaN stores 0.  Stated difference: the hardware's own sRGB
 *              conversion of a colour attachment has a tolerance; this is the rule.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message): width and
 * height not zero; at most 65536 a side; width * height at most 2^32 - 1; source_format 0 or 1; output_format 0, 1 or 2; tonemap_type
 * 0 .. 3; final_attachment aligned to its texel (4 or 8 bytes) with one texel per pixel; dst_attachment 4-byte aligned with one u32 per
 * pixel; with OXC_SCENE_HAS_BLOOM: width and height at least 2, the pyramid's width == W / 2, height == H / 2 and 1 <= levels <= 13,
 * level 0 aligned to its texel and inside the pyramid's `bytes` (the other levels are not looked at); dst_attachment shares no byte with
 * final_attachment, with level 0 of the pyramid or with exposure_buffer (each only when read); with OXC_SCENE_HAS_EYE_ADAPTATION
 * exposure_buffer 4-byte aligned and 8 bytes; every float setting the flags read finite -- exposure without HasEyeAdaptation,
 * bloom_intensity with HasBloom, chromatic_aberration_amount, vignette_amount, film_grain_scale and film_grain_amount with their flags;
 * film_grain_scale > 0 with HasFilmGrain.  Without its flag the pyramid and the exposure buffer are not looked at and may be null.
 * Every other bit of scene_flags is ignored.  One launch, no scratch, no allocation, no host synchronisation; capturable into a HIP
 * graph as one more link of the linear chain. */
#define OXC_SCENE_HAS_FILM_GRAIN (1u << 6) /* GPU::SceneFlags (SceneGPU.hpp:258-266) */
#define OXC_SCENE_HAS_CHROMATIC_ABERRATION (1u << 7)
#define OXC_SCENE_HAS_VIGNETTE (1u << 8)
#define OXC_TONEMAP_NONE 0u /* GPU::TonemapType (SceneGPU.hpp:304-309) */
#define OXC_TONEMAP_ACES 1u
#define OXC_TONEMAP_AGX 2u
#define OXC_TONEMAP_GT7 3u
typedef struct oxc_tonemap_context {
  uint32_t struct_size; /* sizeof(oxc_tonemap_context) */
  uint32_t width, height;
  uint32_t source_format;             /* 0: B10G11R11 UfloatPack32;  1: R16G16B16A16 Sfloat -- the source and the bloom pyramid */
  uint32_t output_format;             /* 0: R8G8B8A8 Srgb;  1: B8G8R8A8 Srgb;  2: R8G8B8A8 Unorm */
  uint32_t scene_flags;               /* HasEyeAdaptation, HasBloom, HasFilmGrain, HasChromaticAberration, HasVignette, TransparentBackground */
  uint32_t tonemap_type;              /* OXC_TONEMAP_* */
  float exposure;                     /* GPU::PostProcessSettings (SceneGPU.hpp:295-302): 1.0; read without HasEyeAdaptation */
  float chromatic_aberration_amount;  /* 0.5 */
  float vignette_amount;              /* 0.5 */
  float film_grain_scale;             /* 1.0 */
  float film_grain_amount;            /* 0.5 */
  uint32_t film_grain_seed;           /* 0 */
  float bloom_intensity;              /* pp.bloom_intensity, what apply_bloom left in PostProcessContext: 0.1 */
  oxc_buffer final_attachment;        /* in: what oxc_apply_pbr wrote */
  oxc_image_pyramid bloom_upsampled_attachment; /* in, read only with OXC_SCENE_HAS_BLOOM: what oxc_apply_bloom wrote; only level 0 is read */
  oxc_buffer exposure_buffer;         /* in, read only with OXC_SCENE_HAS_EYE_ADAPTATION: {f32 adapted_luminance, f32 exposure} */
  oxc_buffer dst_attachment;          /* out: u32[height][width] */
} oxc_tonemap_context;

oxc_status oxc_apply_tonemap(oxc_ctx* ctx, const oxc_tonemap_context* context, void* hip_stream);

/* ---- FXAA: edge anti-aliasing of the lit HDR image ---------------------------------------------------------------------------------
 * Replaces the `fxaa` pass of the reference's post-process chain (Oxylus/src/Render/Shaders/passes/fxaa/fxaa.slang, bound at
 * RendererInstance.cpp:1225-1255 with LinearSamplerClamped of include/Render/Utils/VukCommon.hpp), which runs between apply_pbr and
 * apply_eye_adaptation whenever SceneFlags::HasFXAA is set (RendererInstance.cpp:531-532): the image oxc_apply_pbr wrote goes in, a second
 * image of the same extent and format comes out, and the eye adaptation, the bloom and the tonemap read that one.
 * Out of scope: the atmosphere branch.  The call does not read OXC_SCENE_HAS_FXAA: the C++ shim and the Python twin use it to decide
 * whether the pass runs and which image the later passes read.
 * Arithmetic: the canonical binary32 arithmetic of oxc_apply_pbr -- round to nearest even, left to right, no contraction, IEEE division
 * (1.0 / x is a division) and sqrt, min / max through fminf / fmaxf (a NaN operand gives the other one), clamp(x, a, b) = min(max(x, a), b),
 * lerp(a, b, t) = a + (b - a) * t, abs clears the sign bit; a comparison with a NaN operand is false; a decimal literal is the binary32
 * nearest to it.  The decodes are those of oxc_apply_tonemap step 1: source_format 0 the exact UF11 / UF11 / UF10 decode with alpha 1.0,
 * source_format 1 four halves through binary16 -> binary32, exact, denormals kept.  The checker is tests/fxaa_model.py.
 * Per pixel (x, y) of the W x H image, every statement in the order the Slang writes it:
 *   1. coordinates  tex_coord = ((f32(x) + 0.5) / f32(W), (f32(y) + 0.5) / f32(H));  inverse_screen_size = (1.0f / f32(W), 1.0f / f32(H)).
 *   2. neighbour taps (:24-33, 48-51)  The centre tap and the eight Sample(..., offset) taps sample an image of the output's own extent at a
 *              pixel centre plus an integer offset.  Stated rule, as in oxc_apply_bloom step 4 and oxc_apply_tonemap step 1: a load of
 *              texel (clamp(x + dx, 0, W - 1), clamp(y + dy, 0, H - 1)).  "down" is dy = -1 and "up" dy = +1, "left" dx = -1, as the Slang
 *              writes them.
 *   3. luma      (:19)  luma = sqrt((r * 0.299f + g * 0.587f) + b * 0.114f), of the decoded texel for the nine taps of 2 and of the
 *              bilinear-filtered colour for the samples of 6, as written.  A negative sum (RGBA16F only) gives NaN; every comparison with
 *              a NaN is false, so such a pixel follows the path the Slang's comparisons give it.  No special cases.
 *   4. early out (:36-45)  luma_min = min(center, min(min(down, up), min(left, right))), luma_max likewise with max, luma_range =
 *              luma_max - luma_min; if luma_range < max(0.0312f, luma_max * 0.125f) the pixel's colour is the centre texel's (store, 8).
 *   5. edge      (:53-103)  luma_down_up = down + up, luma_left_right = left + right, left_corners = down_left + up_left, down_corners =
 *              down_left + down_right, right_corners = down_right + up_right, up_corners = up_right + up_left;  edge_horizontal =
 *              (abs(-2.0f * left + left_corners) + abs(-2.0f * center + luma_down_up) * 2.0f) + abs(-2.0f * right + right_corners);
 *              edge_vertical = (abs(-2.0f * up + up_corners) + abs(-2.0f * center + luma_left_right) * 2.0f) + abs(-2.0f * down +
 *              down_corners);  is_horizontal = edge_horizontal >= edge_vertical;  step_length = is_horizontal ? inverse.y : inverse.x;
 *              (luma1, luma2) = is_horizontal ? (down, up) : (left, right);  gradient = luma - center for both;  is1_steepest =
 *              abs(gradient1) >= abs(gradient2);  gradient_scaled = 0.25f * max(abs(gradient1), abs(gradient2));  is1_steepest:
 *              step_length = -step_length and luma_local_average = 0.5f * (luma1 + center), else 0.5f * (luma2 + center);  current_uv =
 *              tex_coord with step_length * 0.5f added to .y (is_horizontal) or .x.
 *   6. search    (:105-161)  offset = is_horizontal ? (inverse.x, 0.0f) : (0.0f, inverse.y);  QUALITY(0 .. 11) = 1, 1, 1, 1, 1, 1.5, 2, 2,
 *              2, 2, 4, 8;  uv1 = current_uv - offset * QUALITY(0), uv2 = current_uv + offset * QUALITY(0);  luma_end1 = luma(Sample(uv1))
 *              - luma_local_average, luma_end2 likewise;  reached1 = abs(luma_end1) >= gradient_scaled, reached2 likewise, reached_both
 *              their conjunction -- computed after the first pair of taps;  then the conditional advance uv1 -= offset * QUALITY(1)
 *              without reached1 and uv2 += offset * QUALITY(1) without reached2;  then, without reached_both, for i = 2 .. 11: a side
 *              not reached samples again (a side that has been reached keeps its last luma_end), both flags are computed anew, a side
 *              not reached advances by offset * QUALITY(i), and reached_both ends the loop.  ITERATIONS is 12.
 *              Every Sample here and in 7 is the manual bilinear of the oxc_apply_bloom block in clamp mode on the W x H source:
 *              g = uv * (f32(W), f32(H)) - 0.5, i = floor(g) converted to i32 saturating (a NaN gives 0), f = g - floor(g), the four
 *              texels (clamp(i.x + {0, 1}, 0, W - 1), clamp(i.y + {0, 1}, 0, H - 1)), lerp(lerp(t00, t10, f.x), lerp(t01, t11, f.x), f.y)
 *              per channel.  The stated difference about hardware samplers is the same.
 *   7. result    (:163-211)  distance1 = is_horizontal ? tex_coord.x - uv1.x : tex_coord.y - uv1.y, distance2 = is_horizontal ? uv2.x -
 *              tex_coord.x : uv2.y - tex_coord.y;  is_direction1 = distance1 < distance2;  distance_final = min(distance1, distance2);
 *              edge_thickness = distance1 + distance2;  is_luma_center_smaller = center < luma_local_average;  correct_variation =
 *              ((is_direction1 ? luma_end1 : luma_end2) < 0.0f) != is_luma_center_smaller;  pixel_offset = (-distance_final) /
 *              edge_thickness + 0.5f;  final_offset = correct_variation ? pixel_offset : 0.0f;  luma_average = k * ((2.0f * (luma_down_up
 *              + luma_left_right) + left_corners) + right_corners) with k = 1.0f / 12.0f as one binary32 constant;  s1 = clamp(abs(
 *              luma_average - center) / luma_range, 0.0f, 1.0f);  s2 = ((-2.0f * s1 + 3.0f) * s1) * s1;  sub_pixel_offset_final = (s2 *
 *              s2) * 0.75f (SUBPIXEL_QUALITY);  final_offset = max(final_offset, sub_pixel_offset_final);  final_uv = tex_coord with
 *              final_offset * step_length added to .y (is_horizontal) or .x;  the pixel's colour is Sample(final_uv), all four channels.
 *   8. store     source_format 0: the truncating UF11 / UF11 / UF10 pack of oxc_decode_visbuffer step 8.  source_format 1: the binary16
 *              conversion of oxc_apply_pbr step 12 for all four channels (a NaN stored as 0x7E00); alpha is the centre texel's alpha on the
 *              early-out path and the bilinear alpha at final_uv otherwise.  The early-out path stores the DECODED centre colour through
 *              the same packers, not a raw copy: a NaN half becomes 0x7E00 there too.  The reference clears the destination first;
 *              every texel is overwritten, so no clear is launched.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message): width and
 * height not zero; at most 65536 a side; width * height at most 2^32 - 1; source_format 0 or 1; final_attachment, then fxaa_attachment,
 * aligned to its texel (4 or 8 bytes) with one texel per pixel; the two images share no byte.  One launch, no scratch, no allocation, no
 * host synchronisation; capturable into a HIP graph as one more link of the linear chain. */
#define OXC_SCENE_HAS_FXAA (1u << 4) /* GPU::SceneFlags (SceneGPU.hpp:259); oxc_apply_fxaa does not read it: the shim and the Python twin do */
typedef struct oxc_fxaa_context {
  uint32_t struct_size; /* sizeof(oxc_fxaa_context) */
  uint32_t width, height;
  uint32_t source_format;       /* 0: B10G11R11 UfloatPack32;  1: R16G16B16A16 Sfloat -- both images */
  oxc_buffer final_attachment;  /* in: what oxc_apply_pbr wrote */
  oxc_buffer fxaa_attachment;   /* out: the same extent and format */
} oxc_fxaa_context;

oxc_status oxc_apply_fxaa(oxc_ctx* ctx, const oxc_fxaa_context* context, void* hip_stream);

/* ---- the sky LUTs of the atmosphere path ------------------------------------------------------------------------------------------------
 * oxc_generate_sky_luts replaces the pair the reference builds once in the RendererInstance constructor (RendererInstance.cpp:136-251:
 * pipelines sky_transmittance and sky_multiscatter; passes/sky_transmittance.slang, passes/sky_multiscattering.slang); an engine calls it
 * again whenever the Atmosphere record changes.  oxc_draw_atmosphere replaces RendererInstance::draw_atmosphere (Passes/PBR.cpp:9-141)
 * without its middle sky_ibl pass, which is oxc_generate_sky_ibl below: pipelines sky_view and sky_aerial_perspective.  All four passes go
 * through sky.slang, bound with LinearSamplerClamped.
 * The consumer of these LUTs and of the sky cubemap is the atmosphere branch of pbr_apply.slang: oxc_apply_pbr_atmosphere (oxc_apply_pbr
 * refuses OXC_SCENE_HAS_ATMOSPHERE).
 * Images: all four are R16G16B16A16 Sfloat, here linear u16x4 buffers of binary16 bits like the normal image, row-major; the 3-D LUT is
 * [depth][height][width].  A store is the binary16 conversion of oxc_apply_pbr step 12 per channel (a NaN stored as 0x7E00).  A
 * SampleLevel(LinearSamplerClamped, uv, 0).rgb is the manual bilinear of the oxc_apply_bloom block in clamp mode on the decoded halves
 * (exact, denormals kept), as oxc_apply_fxaa step 6 states it.  The reference clears the two images of draw_atmosphere first; every texel
 * is written, so no clear is launched.
 * oxc_atmosphere is the byte layout of GPU::Atmosphere (SceneGPU.hpp:158-181: 4-byte alignment, vuk::Extent3D as three u32), 136 bytes.
 * The LUT extents come from the record, as in the Slang; the .z of the three 2-D sizes is not read.
 * Arithmetic: the canonical binary32 arithmetic of oxc_apply_pbr, as oxc_apply_fxaa restates it.  exp(x) is the exp rule of
 * oxc_apply_tonemap step 6, pow(v, p) its pow rule (a base under 2^-126, zero or negative, has log2 -Inf), cos(a) its cos rule.
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; length = sqrt(dot(a, a)); normalize(a) = a / length(a) per component; o + t * d per component
 * with the product first; safe_sqrt(x) = sqrt(max(0, x)); PI and TAU are the binary32 nearest to the Slang's literals.
 * Host constants: what depends on the call's arguments alone is evaluated once per call on the host in binary64 from the binary32
 * arguments (a decimal literal is the binary32 nearest to it, widened; max is fmax), each value rounded to binary32 once:
 *     H = sqrt(max(0, atmos_radius^2 - planet_radius^2))  -- the `h` of sky_transmittance.slang and of transmittance_params_to_lut_uv;
 *     the four constants of henyey_greenstein_draine_phase (common/math.slang:64-68) with g = mie_asymmetry: the argument of each exp
 *     (-(0.0990567 / (g - 1.67154)); -(2.20679 / (g + 3.91029)) - 0.428934; 3.62489 - (8.29288 / (g + 5.52825)); -(0.599085 / (g - 0.641583))
 *     - 0.665888) in binary64, rounded to binary32, then the exp rule: g_hg, g_d, alpha, w_d;
 *     oxc_draw_atmosphere only: eye_altitude = max(camera_position.y * 0.01 + min_altitude, min_altitude), min_altitude = planet_radius +
 *     0.001 (Atmosphere::get_eye_pos; eye_pos = (0, eye_altitude, 0) and h = length(eye_pos) = eye_altitude);  horizon = sqrt(max(0,
 *     h^2 - planet_radius^2)) of the rounded h;  beta = acos(horizon / h), libm's acos of the binary64 quotient;  zenith_horizon_angle = pi -
 *     beta with the binary64 pi.
 * Shared rules, every statement in the Slang's order:
 *   1. intersect  ray_sphere_intersect_nearest(o, d, R): a = dot(d, d), b = 2.0f * dot(d, o), c = dot(o, o) - R * R, delta = b * b - (4.0f
 *              * a) * c;  delta < 0: none.  s0 = (-b + -1.0f * sqrt(delta)) / (2.0f * a), s1 = (-b + sqrt(delta)) / (2.0f * a);  both
 *              negative: none;  s0 < 0: max(0, s1);  s1 < 0: max(0, s0);  else max(0, min(s0, s1)).  Where the Slang reads .value of a
 *              none (the transmittance pass does), the value is 0.0.
 *   2. medium    MediumScattering(altitude): rd = exp(-altitude / rayleigh_density), md = exp(-altitude / mie_density), od = max(0, 1.0f -
 *              abs(altitude - ozone_height) / ozone_thickness);  rayleigh = rayleigh_scatter * rd, mie = mie_scatter * md, me =
 *              mie_extinction * md, ozone = ozone_absorption * od;  scattering_sum = rayleigh + mie;  extinction_sum = (rayleigh + me) +
 *              ozone.  A zero density divides by zero; the exp rule takes what comes (exp(-Inf) = 0, exp(NaN) = NaN).
 *   3. transmittance sample  at (h, mu): rho = safe_sqrt(h * h - planet_radius^2), discriminant = (h * h) * (mu * mu - 1.0f) +
 *              atmos_radius^2, d = max(0, -h * mu + safe_sqrt(discriminant)), d_min = atmos_radius - h, d_max = rho + H, uv = ((d - d_min) /
 *              (d_max - d_min), rho / H), the sample of sky_transmittance_lut there.
 *   4. phases    rayleigh_phase = k * (1.0f + c * c), k = 3.0f / (16.0f * PI) in binary32;  draine_phase(alpha, g, c) = ((1.0f / (4.0f *
 *              PI)) * ((1.0f - g * g) / pow((1.0f + g * g) - (2.0f * g) * c, 1.5f))) * ((1.0f + (alpha * c) * c) / (1.0f + (alpha * (1.0f /
 *              3.0f)) * (1.0f + (2.0f * g) * g)));  mie_phase = lerp(draine_phase(0, g_hg, c), draine_phase(alpha, g_d, c), w_d);  c =
 *              dot(sun_dir, eye_dir).
 *   5. integrate  integrate_single_scattered_luminance (sky.slang:169-256) with luminance = multiscattering_as_1 = 0, transmittance = 1:
 *              dot(eye, eye) <= planet_radius^2 returns that.  planet = intersect(eye, dir, planet_radius).  t_max == -1.0 (the default,
 *              which the multiscattering and the sky-view pass leave) selects the intersection path: atmos = intersect(eye, dir,
 *              atmos_radius); none returns the initial result; length = planet is none ? atmos.value : max(0, planet.value).  The aerial
 *              pass sets t_max, a max(0, ..) or a NaN and so never -1.0: length = t_max.  Then for (step = 0.0f; step < step_count; step
 *              += 1.0f): shift = (length * (step + 0.3f)) / step_count, step_length = shift - the previous shift (0 at first);  pos = eye +
 *              shift * dir, h = length(pos), altitude = h - planet_radius, the medium of 2, up = pos / h, sun_theta = dot(sun_dir, up), T_sun
 *              = the sample of 3 at (h, sun_theta);  MS = 0 -- eval_multiscattering is false in all three callers as the Slang stands
 *              (only the multiscattering pass assigns it, to false), so sky_multiscatter_lut is bound and checked but not read; the kernel
 *              keeps the switch as a template parameter (uv = from_unit_to_sub_uvs(clamp((sun_theta * 0.5f + 0.5f, altitude / (atmos_radius
 *              - planet_radius)), 0, 1)));  phase = mie * mie_phase + rayleigh * rayleigh_phase;  earth_shadow = intersect(pos - 0.001f *
 *              up, sun_dir, planet_radius) is none ? 1 : 0;  sun_luminance = (earth_shadow * T_sun) * phase + MS * scattering_sum;  t =
 *              exp(-step_length * extinction_sum);  integral = (sun_luminance - sun_luminance * t) / extinction_sum, ms_integral =
 *              (scattering_sum - scattering_sum * t) / extinction_sum;  luminance += sun_intensity * (integral * transmittance),
 *              multiscattering_as_1 += ms_integral * transmittance, transmittance *= t.  With eval_planet_luminance, a planet hit and
 *              length == planet.value: pos = eye + length * dir, h, up = pos / h, sun_theta, NoL = saturate(dot(normalize(sun_dir),
 *              normalize(up))), luminance += sun_intensity * ((((T_sun * transmittance) * NoL) * terrain_albedo) / PI).
 *   6. move_to_top_atmosphere(pos, dir): h = length(pos); h > atmos_radius: top = intersect(pos, dir, atmos_radius), none returns
 *              false, else pos = (pos + dir * top.value) + (pos / h) * -0.001f.
 * oxc_generate_sky_luts, texel (x, y) with uv = ((f32(x) + 0.5f) / f32(width), (f32(y) + 0.5f) / f32(height)):
 *   7. transmittance  rho = H * uv.y, lut_x = sqrt(rho * rho + planet_radius^2), d_min = atmos_radius - lut_x, d_max = rho + H, d = d_min +
 *              uv.x * (d_max - d_min), lut_y = d == 0 ? 1.0f : ((H * H - rho * rho) - d * d) / ((2.0f * lut_x) * d) clamped to [-1, 1];
 *              sun_dir = (0, sqrt(1.0f - lut_y * lut_y), lut_y), ray_pos = (0, 0, lut_x), distance_per_step = intersect(ray_pos, sun_dir,
 *              atmos_radius).value / 1000.0f;  1000 times, in this order: ray_pos += sun_dir * distance_per_step, optical_depth +=
 *              extinction_sum(length(ray_pos) - planet_radius) * distance_per_step.  Stored: (exp(-optical_depth), 1.0).
 *   8. multiscatter  altitude = (planet_radius + uv.y * (atmos_radius - planet_radius)) + 0.001f, c = uv.x * 2.0f - 1.0f, sun_dir = (0, c,
 *              safe_sqrt(1.0f - c * c)), eye = (0, altitude, 0);  for each of the 64 caller-supplied directions in ascending order, the
 *              integral of 5 with eval_planet_luminance, step_count 32 and AtmosphereIntegrateInfo's default sun_intensity 10.0; luminance and
 *              multiscattering_as_1 are summed from 0 in that order.  luminance *= (4.0f * PI) * (1.0f / 64.0f), multiscattering_as_1 *=
 *              1.0f / 64.0f, stored: ((luminance * (1.0f / (4.0f * PI))) * (1.0f / (1.0f - multiscattering_as_1)), 1.0).  The table
 *              (HEMISPHERE_64 of the reference's embedded.hemisphere) is the caller's, like the Hilbert table of
 *              oxc_generate_ambient_occlusion: 64 x float3, read as given -- not normalised, not checked.
 * oxc_draw_atmosphere:
 *   9. sky view  uv of the texel as above, then uv_to_sky_view_lut_params: uv = (uv - 0.5f / res) * (res / (res - 1.0f));  uv.y < 0.5f: coord
 *              = uv.y * 2.0f, 1.0f - coord, squared, 1.0f - coord, view_zenith_angle = zenith_horizon_angle * coord;  else coord = uv.y * 2.0f
 *              - 1.0f, squared, view_zenith_angle = zenith_horizon_angle + beta * coord.  longitude = uv.x * TAU;  cz = cos(view_zenith_angle),
 *              sz = safe_sqrt(1.0f - cz * cz) * (view_zenith_angle > 0 ? 1 : -1);  cl = cos(longitude), sl = safe_sqrt(1.0f - cl * cl) *
 *              (longitude <= PI ? 1 : -1);  eye_dir = (sz * cl, cz, sz * sl).  move_to_top_atmosphere(eye_pos, eye_dir) false: the texel is
 *              four zeros.  up = eye_pos / h with the h from before the move, c = dot(sun_dir, up), sun = normalize((safe_sqrt(1.0f - c *
 *              c), c, 0)) -- a non-normalised sun_dir is used as given.  The integral of 5 with step_count 48, without the planet term.
 *              luminance = max(luminance, 0) (a NaN gives 0), an Inf replaced by 0 (com::sanitize);  mult = clamp(max(l.x, max(l.y, l.z)),
 *              HALF_MIN_NORMAL = 6.103515625e-5, HALF_MAX = 65504);  stored: (luminance / mult, mult).
 *  10. aerial    texel (x, y, z): world = mul(inv_projection_view, (2.0f * uv - 1.0f, 1.0f, 1.0f)), rows ((m0 a + m1 b) + m2 c) + m3,
 *              world.xyz / world.w;  world_dir = normalize(world - camera_position);  slice = (f32(z) + 0.5f) * (1.0f / f32(depth)),
 *              squared, times f32(depth);  per_slice_depth = f32(width / depth), the INTEGER division of the two i32 the Slang writes (the
 *              consumer in sky.slang divides floats);  t_max = slice * per_slice_depth.  eye_altitude >= atmos_radius: prev = eye_pos;
 *              move_to_top_atmosphere false: four zeros;  length_to_atmosphere = length(prev - eye_pos);  t_max < length_to_atmosphere: four
 *              zeros;  t_max = max(0, t_max - length_to_atmosphere).  The integral of 5 with sun_dir as given, step_count the FLOAT
 *              max(1.0f, (f32(z) + 1.0f) * 2.0f), that t_max, without the planet term.  Stored: (luminance, (t.x * k + t.y * k) + t.z * k)
 *              with k = 1.0f / 3.0f.  The Slang's start_depth, start_pos and ray_pos feed nothing and are not evaluated.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message): every side of
 * a 2-D LUT the call reads or writes in 2 .. 4096 (from_sub_uvs_to_unit divides by res - 1); oxc_draw_atmosphere: every side of the
 * aerial LUT in 1 .. 4096 and at most 2^26 texels; planet_radius and atmos_radius finite, planet_radius > 0, atmos_radius >
 * planet_radius; every buffer, in the order of the context's fields, non-null, then aligned to 8 bytes, then at least as large as its
 * extent says (hemisphere_directions: 768 bytes), each with a message of its own; no output shares a byte with another output or with an
 * input.  oxc_generate_sky_luts is two
 * launches, oxc_draw_atmosphere two; no scratch, no allocation, no host synchronisation; both are capturable into a HIP graph. */
typedef struct oxc_atmosphere {
  float rayleigh_scatter[3], rayleigh_density;
  float mie_scatter[3], mie_density, mie_extinction, mie_asymmetry;
  float ozone_absorption[3], ozone_height, ozone_thickness;
  float terrain_albedo[3], planet_radius, atmos_radius, aerial_perspective_start_km, aerial_perspective_exposure;
  uint32_t transmittance_lut_size[3], sky_view_lut_size[3], multiscattering_lut_size[3], aerial_perspective_lut_size[3];
} oxc_atmosphere;

typedef struct oxc_sky_lut_context {
  uint32_t struct_size; /* sizeof(oxc_sky_lut_context) */
  uint32_t _pad;
  oxc_atmosphere atmosphere;
  oxc_buffer hemisphere_directions; /* in: 64 x float3, required */
  oxc_buffer sky_transmittance_lut; /* out: u16x4 [transmittance_lut_size.y][.x] */
  oxc_buffer sky_multiscatter_lut;  /* out: u16x4 [multiscattering_lut_size.y][.x] */
} oxc_sky_lut_context;

typedef struct oxc_atmosphere_context {
  uint32_t struct_size; /* sizeof(oxc_atmosphere_context) */
  uint32_t _pad;
  oxc_atmosphere atmosphere;
  float sun_dir[3], sun_intensity;       /* directional_light.direction, .intensity */
  float camera_position[3], _pad1;       /* GPU::Camera::position.xyz */
  float camera_inv_projection_view[16];  /* GPU::Camera::inv_projection_view, column-major */
  oxc_buffer sky_transmittance_lut;      /* in: what oxc_generate_sky_luts wrote */
  oxc_buffer sky_multiscatter_lut;       /* in (bound, not read: step 5) */
  oxc_buffer sky_view_lut;               /* out: u16x4 [sky_view_lut_size.y][.x], the engine's 312 x 192 */
  oxc_buffer sky_aerial_perspective_lut; /* out: u16x4 [aerial_perspective_lut_size.z][.y][.x], the engine's 32 x 32 x 32 */
} oxc_atmosphere_context;

oxc_status oxc_generate_sky_luts(oxc_ctx* ctx, const oxc_sky_lut_context* context, void* hip_stream);
oxc_status oxc_draw_atmosphere(oxc_ctx* ctx, const oxc_atmosphere_context* context, void* hip_stream);

/* ---- the sky cubemap of the atmosphere path ---------------------------------------------------------------------------------------------
 * oxc_generate_sky_ibl is the middle pass of RendererInstance::draw_atmosphere (Passes/PBR.cpp:52-94, passes/sky_ibl.slang): from the
 * sky-view LUT oxc_draw_atmosphere wrote and the transmittance LUT it writes sky_cubemap, the image pbr_apply.slang samples for the ambient
 * term.  With it the reference's draw_atmosphere is oxc_draw_atmosphere, then this call (three with oxc_generate_sky_luts, which the
 * reference runs at construction); the aerial LUT and the cube do not read each other.  The consumer is the atmosphere branch of pbr_apply.slang:
 * oxc_apply_pbr_atmosphere.
 * Images: the cube is R16G16B16A16 Sfloat, here a linear u16x4 buffer [6][cube_size][cube_size] like the LUTs; face f is the Slang's
 * thread_id.z, texel (x, y) of it thread_id.xy.  The cube is read and written: a texel is its own history.  The reference clears it to
 * black once, in the constructor (RendererInstance.cpp:187-201); here the caller zeroes the buffer once and the call never clears it.
 * frame_index (render_context->num_frames) travels by value, like the sun of oxc_draw_atmosphere: a captured graph replays the index it
 * was captured with -- every replay still accumulates into the cube, which is memory, but with the sample rotation of that one index; an
 * engine that wants the rotation to advance captures again or updates the node's arguments.
 * Arithmetic and shared rules: those of the block above (steps 1 - 10): intersect (1), the clamp bilinear SampleLevel (here .rgba: the
 * alpha is interpolated like a colour channel), the transmittance sample of 3, the binary16 store, the exact half decode, dot, length,
 * normalize, the cos rule.  cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), each product rounded before the
 * subtraction; a 2-D dot is a.x b.x + a.y b.y; frac(x) = x - floor(x); lerp(a, b, t) = a + (b - a) * t; f32(u32) rounds to nearest even;
 * every decimal literal (0.61803398875, 2.3283064365386963e-10, 0.06711056, 0.00583715, 52.9829189, 0.999, 1e-5, 1e-20, 0.02, 37.0, 17.0)
 * is the binary32 nearest to it.  sanitize(v) is 0 for each non-finite component.
 * Host constants: eye_altitude, horizon, beta and zenith_horizon_angle, the ones of oxc_draw_atmosphere, from camera_position.y; H.
 *  11. closed forms  A(y, x), the atan2 of two binary64: ax = |x|, ay = |y|, a = min(ax, ay) / max(ax, ay);  a > 0x1.a827999fcef32p-2
 *              (sqrt(2) - 1): t = (a - 1) / (a + 1), else t = a;  z = t * t;  p = 1/39, then p = c - p * z for c = 1/37, 1/35, .. 1/3, 1 (the
 *              binary64 quotients; 20 terms);  r = t * p;  reduced: r = pi/4 + r;  ay > ax: r = pi/2 - r;  x < 0: r = pi - r;  y < 0: r = -r
 *              (a negative zero counts as positive in both tests);  max(ax, ay) == 0: r = 0;  a NaN argument gives NaN, as do two infinite
 *              ones (Inf / Inf).  pi = 0x1.921fb54442d18p+1 and its exact half and quarter.  All of it in binary64 without contraction.
 *              atan2(y, x) = (float)A((double)y, (double)x).  acos(x) = (float)A(sqrt(1 - xd * xd), xd) with xd = (double)x -- xd * xd is
 *              exact -- and NaN for a NaN and for |x| > 1;  acos(1) = 0, acos(-1) = (float)pi, acos(0) = (float)(pi/2).  The binary64 value
 *              is within 10 roundings of 2^-53 each (1.2e-15 relative) of the true one, so the result is the correctly rounded binary32 or, where the true value lies that
 *              close to a rounding boundary, its neighbour: at most 1 ulp from the correctly rounded value.
 *              sin(a): the turn t of the cos rule (u = (double)|a| / (2 pi), t = (float)(u - floor(u)), t == 1 becomes 0), the sine of that
 *              turn by the rotation rule of oxc_resolve_shadowmap, negated for a < 0;  NaN for a non-finite a.
 *              rsqrt(x) = 1.0f / sqrt(x) in binary32.
 *  12. texel frame  uv = (f32(pixel) + 0.5f) / f32(cube_size);  v = (uv.x * 2.0f - 1.0f, uv.y * 2.0f - 1.0f, -1.0f);  M =
 *              CUBE_MAP_FACE_ROTATION(face), whose nine scalars fill M ROW by row in the constructor's order (row r = scalars 3 r .. 3 r + 2)
 *              and mul(M, v).r = (M[r][0] v.x + M[r][1] v.y) + M[r][2] v.z, every product formed even where the scalar is 0 or 1: at
 *              cube_size 1 faces 0 .. 5 look along +X, -X, +Y, -Y, +Z, -Z (the transposed convention would swap faces 2 and 3).
 *              output_dir = normalize(mul(M, v));  eye_pos = (0, eye_altitude, 0);  up = |output_dir.y| < 0.999f ? (0, 1, 0) : (1, 0, 0);
 *              tangent = normalize(cross(up, output_dir)), bitangent = cross(output_dir, tangent).  history = the decoded texel;
 *              has_history = history.a > 0 and the three colours finite: a positive denormal alpha is history, -0, a NaN and negatives
 *              are not.  p = (f32(x) + f32(face) * 37.0f, f32(y) + f32(face) * 17.0f), base_rotation = frac(52.9829189f * frac(p.x *
 *              0.06711056f + p.y * 0.00583715f));  rotation = has_history ? frac(base_rotation + f32(frame_index) * 0.61803398875f) :
 *              base_rotation.
 *  13. sample i of 0 .. 63:  u1 = (f32(i) + 0.5f) / 64.0f;  radical_inverse_vdc(i) = f32(the 32-bit reversal of i) *
 *              2.3283064365386963e-10f;  u2 = frac(that + rotation);  r = sqrt(u1), phi = TAU * u2;  local = (r * cos(phi), r * sin(phi),
 *              sqrt(max(0, 1.0f - u1)));  input_dir = normalize((local.x * tangent + local.y * bitangent) + local.z * output_dir).
 *  14. illuminance along input_dir (get_atmosphere_illuminance_along_ray, sky.slang:296-322, as written, whatever it simplifies to):
 *              height = length(eye_pos), up_vec = eye_pos / height, c = dot(input_dir, up_vec);  side_raw = cross(up_vec, input_dir), side
 *              = length(side_raw) > 1e-5f ? normalize(side_raw) : (1, 0, 0);  forward = normalize(cross(side, up_vec));  sun =
 *              normalize(sun_dir);  l = (dot(sun, forward), dot(sun, side)), len_sq = dot(l, l), light_on_plane = len_sq > 1e-20f ? l *
 *              rsqrt(len_sq) : (1, 0) -- the comparison is false for a NaN;  hit = intersect(eye_pos, input_dir, planet_radius) has a value.
 *              sky_view_params_to_lut_uv (sky.slang:39-67) with the host constants: angle = acos(c);  no hit: coord = angle /
 *              zenith_horizon_angle, 1.0f - coord, safe_sqrt, 1.0f - coord, uv.y = coord * 0.5f;  hit: coord = (angle -
 *              zenith_horizon_angle) / beta, safe_sqrt, uv.y = coord * 0.5f + 0.5f.  theta = atan2(-light_on_plane.y, -light_on_plane.x),
 *              uv.x = (theta + PI) / (2.0f * PI);  uv = (uv + 0.5f / res) * (res / (res + 1.0f)), res = f32(sky_view_lut_size.xy).  s =
 *              SampleLevel(sky_view_lut, uv);  the sample is sanitize(s.rgb * s.a) (the Slang sanitizes it a second time in its loop: the
 *              identity).
 *  15. the texel   frame_sum adds the 64 samples from 0 in ascending i;  frame_estimate = frame_sum / 64.0f.  sun_cos_zenith = (sun_dir.x
 *              * 0.0f + sun_dir.y * 1.0f) + sun_dir.z * 0.0f -- sun_dir as given, not normalised;  sun_color = the sample of 3 at
 *              (eye_pos.y, sun_cos_zenith);  sun_facing = saturate(dot(output_dir, sun_dir));  sun_term = (((sun_ambient_strength *
 *              sun_color) * sun_intensity) * sun_facing) / PI.  frame_result = clamp(sanitize(frame_estimate + sun_term), 0, HALF_MAX), the
 *              clamp as two selects after the sanitize: v > 0 ? v : +0, then v < 65504 ? v : 65504.  Stored: (has_history ?
 *              lerp(history.rgb, frame_result, 0.02f) : frame_result, 1.0).  No stored half is a NaN or an Inf, whatever the arguments.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its
 * own): struct_size; every side of sky_view_lut_size, then of transmittance_lut_size, in 2 .. 4096; cube_size in 1 .. 1024;
 * planet_radius and atmos_radius finite, planet_radius > 0, atmos_radius > planet_radius; every buffer, in the order of the context's
 * fields, non-null, then aligned to 8 bytes, then at least as large as its extent says; the cube shares no byte with either LUT.
 * One launch; no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
typedef struct oxc_sky_ibl_context {
  uint32_t struct_size; /* sizeof(oxc_sky_ibl_context) */
  uint32_t _pad;
  oxc_atmosphere atmosphere;
  float sun_dir[3], sun_intensity;                /* directional_light.direction, .intensity */
  float camera_position[3], sun_ambient_strength; /* GPU::Camera::position.xyz; the engine passes 0.15f */
  uint32_t frame_index;                           /* render_context->num_frames */
  uint32_t cube_size;                             /* the engine's 32 (IBL_CUBE_RES); 64 samples per texel and call */
  oxc_buffer sky_view_lut;                        /* in: what oxc_draw_atmosphere wrote */
  oxc_buffer sky_transmittance_lut;               /* in: what oxc_generate_sky_luts wrote */
  oxc_buffer sky_cubemap;                         /* in and out: u16x4 [6][cube_size][cube_size]; zeroed once by the caller */
} oxc_sky_ibl_context;

oxc_status oxc_generate_sky_ibl(oxc_ctx* ctx, const oxc_sky_ibl_context* context, void* hip_stream);

/* ---- PBR apply, the atmosphere branch: the lit HDR image with the sky, the sun disc, aerial perspective and the sky-lit ambient ----------------
 * Replaces the atmosphere branch of RendererInstance::apply_pbr (Oxylus/src/Render/Passes/PBR.cpp:318-434, pipeline pbr_apply,
 * passes/pbr_apply.slang with pbr.slang, sky.slang and scene.slang): the consumer of what oxc_generate_sky_luts, oxc_draw_atmosphere and
 * oxc_generate_sky_ibl wrote.  A call of its own with a context of its own: oxc_apply_pbr keeps its layout and keeps refusing
 * OXC_SCENE_HAS_ATMOSPHERE; here that bit may be set or clear (it is the caller's dispatch bit and is not read).  The call reads
 * OXC_SCENE_HAS_DIRECTIONAL_LIGHT, OXC_SCENE_HAS_CONTACT_SHADOWS and OXC_SCENE_TRANSPARENT_BACKGROUND.
 * Not in the context: base_ambient_color and the GPU::Sky record.  In pbr_apply.slang diffuse_sky and specular_sky start as
 * base_ambient_color and are overwritten on every lit pixel (:139-140), and has_sky (:93) feeds nothing.
 * Arithmetic: every device operation in the canonical binary32 arithmetic oxc_apply_pbr states; the four sky images are u16x4 buffers in
 * the layouts their producers write, a SampleLevel(LinearSamplerClamped) of one is the clamp bilinear of the sky LUT block; "atmosphere
 * step n" is step n of that block, "step n" alone step n of oxc_apply_pbr.
 * Host constants, once per call: eye_altitude, beta and zenith_horizon_angle as oxc_draw_atmosphere forms them from camera_position.y, and H;
 * in binary32 operations: min_altitude = planet_radius + 0.001f;  sun_cos_theta = (L.x * 0.0f + L.y * 1.0f) + L.z * 0.0f, L = sun_dir as
 * given;  horizon_darkening = smoothstep(-0.1f, 0.3f, sun_cos_theta) by the stated smoothstep;  min_cos = the cos rule of oxc_apply_pbr at
 * (1.0f * PI) / 180.0f;  lut = f32(aerial_perspective_lut_size);  per_slice_depth = lut.x / lut.z, the FLOAT quotient (sky.slang:266; the
 * producer's integer quotient differs where x is no multiple of z: both are as written);  1.0f / per_slice_depth, 1.0f / lut.z, 1.0f / 0.001f.
 * Per pixel (x, y):
 *   A. transparent, decode, position, frame  (pbr_apply.slang:50-83)  steps 1 - 4, unchanged.
 *   B. visibility  (:85-87)  directional_shadow and contact_shadow as in step 6; an image whose flag is clear is not read, not checked and may
 *              be null.
 *   C. sun  (:97-106)  for every pixel that passed A, the empty ones included:  world_eye_y = max(world.y * 0.01f + min_altitude,
 *              min_altitude), a per-pixel binary32 value (max is fmaxf: a NaN world.y gives min_altitude);  sun_transmittance = the
 *              transmittance sample of atmosphere step 3 at (world_eye_y, sun_cos_theta);  direct = (sun_transmittance * Li) *
 *              horizon_darkening per channel.  direct does not depend on HasDirectionalLight, only directional_shadow does: that is what
 *              the Slang says.  A non-finite world (h.w == 0) runs on: the IEEE results and the clamp bilinear's defined behaviour for a
 *              NaN coordinate are the rule.
 *   D. sky pixel  (depth == 0.0, :108-124)  h = eye_altitude, eye_pos = (0, h, 0);  up = (0, 1, 0);  right = normalize(cross(up, -V));
 *              forward = normalize(cross(right, up));  l = (dot(L, forward), dot(L, right));  light_on_plane = l / sqrt(l.x * l.x + l.y *
 *              l.y), the plain 2-D normalize and not atmosphere step 14's safe_normalize: a zero l gives NaN, and the NaN goes through
 *              atan2;  c = dot(-V, up), every product formed;  hit = intersect(eye_pos, -V, planet_radius) has a value;  uv =
 *              sky_view_params_to_lut_uv exactly as atmosphere step 14 states it (acos and atan2 by step 11);  s = the .rgba sample of
 *              sky_view_lut at uv.  No hit:  s.rgb += (draw_sun(-V, L) * Li) * sun_transmittance, where draw_sun (:26-38) is: ct = dot(-V, L);
 *              ct >= min_cos gives 1.0 (a NaN takes the other arm);  otherwise offset = min_cos - ct, g = exp(-offset * 50000.0f) * 0.5f by
 *              the exp rule, inv = (1.0f / (0.02f + offset * 300.0f)) * 0.01f, g + inv.  The colour is s.rgb * s.a, alpha 1, and the pixel
 *              is done.  The sun_transmittance is C's, from this pixel's world, as written.
 *   E. aerial perspective  (:127-133, sky.slang:258-293)  rel = (world - camera_position) * 0.01f per component;  relative_depth = max(0,
 *              length(rel) - aerial_perspective_start_km);  linear_slice = relative_depth * (1.0f / per_slice_depth);  linear_w =
 *              linear_slice * (1.0f / lut.z);  non_linear_w = sqrt(linear_w);  non_linear_slice = non_linear_w * lut.z;  weight = 1, and
 *              with non_linear_slice < 0.70710678118654752f weight = saturate((non_linear_slice * non_linear_slice) * 2.0f);  weight =
 *              weight * saturate(relative_depth * (1.0f / 0.001f)).  a = the clamp trilinear sample at (uv of step 3, non_linear_w): the third
 *              axis by the same axis rule on non_linear_w with the LUT's depth, the bilinear .rgba of slice i0 and of slice i1, then lerp
 *              by the z weight.  a.rgb *= weight;  a.w = 1.0f - (weight * (1.0f - a.w));  a.rgb *= aerial_perspective_exposure;  aerial =
 *              a.rgb * a.w.
 *   F. cube sample of a direction r (a stated rule, like the albedo sampler's)  ax = |r.x|, ay = |r.y|, az = |r.z|;  az >= ax && az >= ay
 *              selects Z, else ay >= ax selects Y, else X (a NaN makes a comparison false);  the sign of the major component picks the
 *              face of the pair, a negative zero or a NaN counting as positive;  (face, sc, tc, ma) by the Vulkan table: +X (0, -r.z, -r.y,
 *              r.x), -X (1, +r.z, -r.y, r.x), +Y (2, r.x, +r.z, r.y), -Y (3, r.x, -r.z, r.y), +Z (4, r.x, -r.y, r.z), -Z (5, -r.x, -r.y,
 *              r.z) -- the inverse of step 12's row-major CUBE_MAP_FACE_ROTATION of oxc_generate_sky_ibl;  s = (sc / |ma|) * 0.5f + 0.5f, t
 *              likewise;  the sample is the clamp bilinear .rgba of that face alone at (s, t).  Stated deviation: the hardware filters
 *              seamlessly across face edges, this rule clamps inside the face; the two differ only within half a texel of an edge.
 *   G. sky ambient  (:135-140)  reflection_dir = normalize(lerp(N, R, 1.0f - roughness));  spec = cube(reflection_dir), diff = cube(N);
 *              specular_sky = (spec.rgb * spec.a) * horizon_darkening, diffuse_sky likewise.
 *   H. surface, ambient  (:143-157)  steps 7 and 8 with env replaced per channel: ibl_diffuse = ((kD * diffuse_sky) * albedo) *
 *              Fd_Lambert(), ibl_specular = (kS * specular_sky) * spec_occlusion.
 *   I. lights, BRDF  steps 9 and 10, unchanged.
 *   J. sun term  step 11 with direct per channel: surface = (((b.diffuse + b.specular * horizon) * direct_c) * NoL) * visibility.
 *   K. store  colour = (((surface + total) + indirect) + emission) + aerial;  formats and NaN handling as step 12.
 * Limits (else OXC_INVALID_ARG, nothing launched, the output untouched; the first broken rule in this order gives the message, each has its
 * own): struct_size; the extent rules of oxc_apply_pbr; every side of transmittance_lut_size, then of sky_view_lut_size, in 2 .. 4096; every
 * side of the aerial LUT in 1 .. 4096 and at most 2^26 texels; cube_size in 1 .. 1024; planet_radius and atmos_radius finite, planet_radius
 * > 0, atmos_radius > planet_radius; aerial_perspective_start_km and aerial_perspective_exposure finite; every host scalar (the matrix,
 * camera_position, sun_dir, sun_intensity) finite; the G-buffer, shadow and light rules of oxc_apply_pbr; the four sky buffers in field
 * order, each non-null, then aligned to 8 bytes, then at least as large as its extent says; final_attachment as in oxc_apply_pbr, sharing
 * no byte with any input.  One launch, no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
typedef struct oxc_pbr_atmosphere_context {
  uint32_t struct_size; /* sizeof(oxc_pbr_atmosphere_context) */
  uint32_t width, height;
  uint32_t scene_flags;           /* GPU::SceneFlags */
  uint32_t light_count;
  float inv_projection_view[16];  /* Camera::inv_projection_view, column-major */
  float camera_position[3];
  float sun_dir[3];               /* L: towards the sun, used as given */
  float sun_intensity;            /* Li */
  oxc_atmosphere atmosphere;      /* the record the three producers were called with */
  uint32_t cube_size;             /* the engine's 32 */
  uint32_t _pad;
  oxc_image depth_attachment;     /* the next nine: as in oxc_pbr_context */
  oxc_buffer albedo_attachment;
  oxc_buffer normal_attachment;
  oxc_buffer emissive_attachment;
  oxc_buffer metallic_roughness_occlusion_attachment;
  oxc_buffer ambient_occlusion_attachment;
  oxc_image resolved_shadows_attachment;
  oxc_image contact_shadows_attachment;
  oxc_buffer lights_buffer;
  oxc_buffer sky_transmittance_lut;      /* in: u16x4 [transmittance_lut_size.y][.x], what oxc_generate_sky_luts wrote */
  oxc_buffer sky_view_lut;               /* in: u16x4 [sky_view_lut_size.y][.x], what oxc_draw_atmosphere wrote */
  oxc_buffer sky_aerial_perspective_lut; /* in: u16x4 [aerial_perspective_lut_size.z][.y][.x], what oxc_draw_atmosphere wrote */
  oxc_buffer sky_cubemap;                /* in: u16x4 [6][cube_size][cube_size], what oxc_generate_sky_ibl wrote */
  oxc_buffer final_attachment;    /* out: u32[height][width] B10G11R11, or u16x4[height][width] with a transparent background */
} oxc_pbr_atmosphere_context;

oxc_status oxc_apply_pbr_atmosphere(oxc_ctx* ctx, const oxc_pbr_atmosphere_context* context, void* hip_stream);

/* ---- the terrain maps: height, ridge, normal, splat and the per-patch min/max ---------------------------------------------------------------
 * oxc_generate_terrain_maps is the three compute passes Terrain::bake (Scene/Terrain.cpp:406-461) runs over the whole map and
 * RendererInstance::apply_terrain_brush (Passes/Terrain.cpp:134-156) runs again over a region: passes/terrain_generate.slang with terrain.slang,
 * passes/terrain_derive.slang and passes/terrain_minmax.slang.  They produce what the terrain consumers read: the heightmap
 * (terrain_visbuffer.slang), the normal and splat maps (terrain_decode.slang) and patch_minmax, the image oxc_cull_terrain takes.  `stages`
 * selects them; the selected ones run in the order generate, derive, minmax on the stream, each seeing what the one before wrote.
 * Images: linear row-major buffers, texel (x, y) at element y * resolution.x + x.  heightmap R16 Unorm (u16), ridgemap R16 Sfloat (u16 of
 * binary16 bits), normalmap R16G16 Sfloat (u16 x 2, .x first), splatmap R8G8B8A8 Unorm (u32, .x in the low byte), height_edit R32 Sfloat,
 * splat_edit R8G8B8A8 Unorm.  Stated deviation: patch_minmax, R16G16 Unorm in the reference, is here the RG32F oxc_image that
 * oxc_terrain_context.patch_minmax_attachment takes (one level, patch (x, y) at float pair y * patch_count.x + x); each float is exactly
 * what a load of the Unorm texel returns, f32(q) / 65535.0f, so the image goes to oxc_cull_terrain as it is.
 * region: 16 bytes of GPU::TerrainRegion {texel_origin.xy, patch_origin.xy} in DEVICE memory, read by the kernels (the brush trace writes it
 * on the GPU); a null buffer means both origins are zero, which is what bake passes.
 * What a call writes: generate and derive the texels texel_origin + [0, roundup(dispatch_texels, 16)) clipped to resolution, minmax the patches
 * patch_origin + [0, roundup(dispatch_patches, 8)) clipped to patch_count: the reference's whole work groups.  Every other byte of every
 * image is left as it was.  origin + index is a u32 sum.  Stated deviation: an index beyond roundup(resolution, 16) (roundup(patch_count, 8))
 * can land inside the map only by that sum wrapping past 2^32; such indices are not launched.
 * Arithmetic: binary32, the expressions of the Slang left to right, one rounding per operation, no contraction, IEEE division and square
 * root; every decimal literal is the binary32 nearest to it (0.3183099, 0.3678794, 0.06711056, 0.00583715, 0.01111, 1e-10, 0.6, TAU =
 * 6.283185307179586476925286766559, ..).  Shared rules, the ones of the blocks above: saturate(x) = min(max(x, 0), 1) and clamp(x, lo, hi) =
 * min(max(x, lo), hi) with fmin / fmax (a NaN gives the lower bound), max(a, b) = fmax, lerp(a, b, t) = a + (b - a) * t, frac(x) = x -
 * floor(x), sign(x) = x > 0 ? 1 : x < 0 ? -1 : 0, smoothstep(e0, e1, x): s = saturate((x - e0) / (e1 - e0)), (s * s) * (3.0f - 2.0f * s);  a
 * 2-D dot is a.x b.x + a.y b.y, a 3-D one (a.x b.x + a.y b.y) + a.z b.z, length = sqrt(dot(v, v)), normalize = v / length;  exp by the exp
 * rule of oxc_apply_tonemap, pow by the pow rule of oxc_apply_pbr, (cos, sin) of a binary32 angle by the rule of oxc_generate_sky_ibl step 11
 * (its binary64 turn reduction holds for every finite angle; a non-finite one gives NaN);  a binary16 store rounds to nearest even, keeps
 * denormals and writes every NaN as 0x7E00; a binary16 load is exact;  unorm8(e) = u32(floor(saturate(e) * 255.0f + 0.5f)), unorm16(e) the
 * same with 65535.0f, their loads f32(q) / 255.0f and f32(q) / 65535.0f;  f32(u32) rounds to nearest even;  seed + i wraps in u32.
 * The host may evaluate what depends on the call alone, once, by the same binary32 operations (strength * scale, 1.0f / (scale *
 * cell_scale), f32(resolution), 1.0f - normalization, height_amplitude * 0.6f, 8.0f * texel_world_size, the minmax scale).
 * E = settings.erosion, G = settings (oxc_terrain_generate), D = oxc_terrain_derive.
 *   T1. texel   texel = texel_origin + thread;  any(texel >= resolution) writes nothing.  uv = (f32(texel) + 0.5f) / f32(resolution);  p = uv *
 *              G.domain_size.
 *   T2. hash2(x, seed)   k = (0.3183099f, 0.3678794f);  so = (f32(seed) * 0.06711056f, f32(seed) * 0.00583715f);  q = ((x.x + so.x) * k.x +
 *              k.y, (x.y + so.y) * k.y + k.x);  t = frac((q.x * q.y) * (q.x + q.y));  hash2 = (-1.0f + 2.0f * frac((16.0f * k.x) * t), -1.0f +
 *              2.0f * frac((16.0f * k.y) * t)).
 *   T3. noised(p, seed)   i = floor(p), f = p - i;  per component u = ((f * f) * f) * (f * (f * 6.0f - 15.0f) + 10.0f), du = ((30.0f * f) * f) *
 *              (f * (f - 2.0f) + 1.0f);  ga, gb, gc, gd = hash2 at i + (0, 0), (1, 0), (0, 1), (1, 1);  va = dot(ga, f), vb = dot(gb, f - (1,
 *              0)), vc = dot(gc, f - (0, 1)), vd = dot(gd, f - (1, 1));  k = ((va - vb) - vc) + vd;  value = ((va + u.x * (vb - va)) + u.y *
 *              (vc - va)) + (u.x * u.y) * k;  derivative.c = (((ga.c + u.x * (gb.c - ga.c)) + u.y * (gc.c - ga.c)) + (u.x * u.y) * (((ga.c -
 *              gb.c) - gc.c) + gd.c)) + du.c * ((w.c * k + v.c) - va) with (w, v).x = (u.y, vb), (w, v).y = (u.x, vc).
 *   T4. fractal_noise   r = (0, 0, 0), amplitude = 1, freq = G.height_frequency;  for i in 0 .. G.height_octaves - 1: o = noised(p * freq,
 *              E.seed + i);  r.x = r.x + o.x * amplitude;  r.yz = r.yz + o.yz * (amplitude * freq);  amplitude = amplitude * G.height_gain;
 *              freq = freq * G.height_lacunarity.
 *   T5. base   base = r * G.height_amplitude;  fade_target = clamp(base.x / (G.height_amplitude * 0.6f), -1, 1);  base.x = base.x * 0.5f +
 *              0.5f.
 *   T6. erosion, before the octaves   clamp01 = saturate;  ease_out(t): v = 1.0f - clamp01(t), 1.0f - v * v;  smooth_start(t, s) = t >= s ? t -
 *              0.5f * s : ((0.5f * t) * t) / s (a NaN takes the second arm);  pow_inv(t, w) = 1.0f - pow(1.0f - clamp01(t), w).
 *              strength = E.strength * E.scale;  target = clamp(fade_target, -1, 1);  height = base.x;  freq = 1.0f / (E.scale *
 *              E.cell_scale);  slope_length = max(length(base.yz), 1e-10f);  magnitude = 0;  rounding_mult = 1;  rounding_for_input =
 *              lerp(E.rounding.y, E.rounding.x, clamp01(target + 0.5f)) * E.rounding.z;  combi_mask = ease_out(smooth_start(slope_length *
 *              E.onset.x, rounding_for_input * E.onset.x));  ridge_mask = ease_out(slope_length * E.onset.z);  ridge_target = target;
 *              gully_slope = lerp(base.yz, (base.yz / slope_length) * E.assumed_slope.x, E.assumed_slope.y) per component.
 *   T7. phacelle(pp, seed), for octave i of 0 .. E.octaves - 1 with pp = p * freq and seed = E.seed + i:   len = length(gully_slope), n = len
 *              > 1e-10f ? gully_slope / len : (0, 0);  side = (((n.y * -1.0f) * E.cell_scale) * TAU, ((n.x * 1.0f) * E.cell_scale) * TAU);
 *              phase_offset = 0.25f * TAU;  c = floor(pp), f = pp - c;  phase_dir = (0, 0), weight_sum = 0;  for a in -1 .. 2, inside it
 *              for b in -1 .. 2 (16 cells, b fastest): g = (f32(a), f32(b));  d = (f - g) - hash2(c + g, seed) * 0.5f;  sq = dot(d, d);
 *              weight = max(0, exp((-sq) * 2.0f) - 0.01111f);  weight_sum = weight_sum + weight;  w = dot(d, side) + phase_offset;
 *              phase_dir = phase_dir + (cos(w) * weight, sin(w) * weight).  interpolated = phase_dir / max(weight_sum, 1e-10f);
 *              magnitude_p = max(1.0f - E.normalization, length(interpolated));  ph.xy = interpolated / magnitude_p, ph.zw = side.
 *   T8. the octave   ph.zw = ph.zw * (-freq);  sloping = |ph.y|;  gully_slope = gully_slope + ((sign(ph.y) * ph.zw) * strength) *
 *              E.gully_weight;  gx = ph.x;  faded = lerp(target, gx * E.gully_weight, combi_mask);  height = height + faded * strength;
 *              magnitude = magnitude + strength;  target = faded;  rounding_for_octave = lerp(E.rounding.y, E.rounding.x, clamp01(ph.x +
 *              0.5f)) * rounding_mult;  new_mask = ease_out(smooth_start(sloping * E.onset.y, rounding_for_octave * E.onset.y));
 *              combi_mask = pow_inv(combi_mask, E.detail) * new_mask;  ridge_target = lerp(ridge_target, gx, ridge_mask);  ridge_mask =
 *              ridge_mask * ease_out(sloping * E.onset.w);  strength = strength * E.gain;  freq = freq * E.lacunarity;  rounding_mult =
 *              rounding_mult * E.rounding.w.  (The Slang also accumulates the slope delta, which nothing reads.)
 *   T9. store   delta = height - base.x;  ridge = ridge_target * (1.0f - ridge_mask);  offset = lerp(G.height_offset.x, -fade_target,
 *              G.height_offset.y) * magnitude;  h = (base.x + delta) + offset;  heightmap = unorm16(h + height_edit[texel]);  ridgemap = the
 *              binary16 store of ridge.
 *   T10. derive   load_height(c) = the unorm16 load at c clamped to [0, resolution - 1] per axis: the heightmap as it is AFTER the generate
 *              stage of the same call, and for a neighbour outside the written region whatever the buffer held.  h00 .. h22 the eight
 *              neighbours, first index x, 0 = -1.  dhdx = ((((h20 + 2.0f * h21) + h22) - ((h00 + 2.0f * h01) + h02)) * D.height_range) / (8.0f *
 *              D.texel_world_size.x);  dhdz = ((((h02 + 2.0f * h12) + h22) - ((h00 + 2.0f * h10) + h20)) * D.height_range) / (8.0f *
 *              D.texel_world_size.y);  normal = normalize((-dhdx, 1.0f, -dhdz));  normalmap = the binary16 stores of (normal.x, normal.z).
 *   T11. splat   height = load_height(texel), ridge = the binary16 load;  slope = saturate(1.0f - normal.y);  rock =
 *              smoothstep(D.slope_rock_begin, D.slope_rock_end, slope);  snow = smoothstep(D.altitude_snow_begin, D.altitude_snow_end,
 *              height) * (1.0f - rock);  drainage = (saturate((-ridge) * D.ridge_drainage_scale) * (1.0f - rock)) * (1.0f - snow);  grass =
 *              saturate(((1.0f - rock) - snow) - drainage);  procedural = (grass, rock, drainage, snow);  painted = the four unorm8 loads of
 *              splat_edit;  painted_weights = (saturate(((1.0f - painted.x) - painted.y) - painted.z), painted.x, painted.y, painted.z);
 *              splatmap = unorm8 of lerp(procedural, painted_weights, painted.w) per component.
 *   T12. minmax   patch = patch_origin + thread;  any(patch >= patch_count) writes nothing.  scale = f32(resolution) / f32(patch_count);
 *              begin = u32(floor(f32(patch) * scale));  end = min(u32(ceil(f32(patch + 1) * scale)) + 1, resolution);  bounds = (1.0, 0.0),
 *              then min / max with the unorm16 load of every texel of [begin, end) on both axes (the seed takes part; min and max of such
 *              values do not depend on the order).  patch_minmax = bounds.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its own):
 * struct_size; stages non-zero with no unknown bit; every side of resolution in 1 .. 16384, then of patch_count in 1 .. 4096;
 * generate.resolution and derive.resolution equal to resolution; generate.height_octaves and generate.erosion.octaves at most 16 (this limit
 * is the library's: the Slang has none, and an unbounded loop count would be a hang); erosion.detail finite and above 0, the pow rule's
 * domain; every buffer a requested stage touches, in the order of the context's fields, non-null (region may be null), then aligned to its
 * texel (region and patch_minmax to 8 bytes), then at least as large as its extent says (patch_minmax: one level at offset 0 of
 * patch_count's extent); no written image shares a byte with another buffer the requested stages touch.  Every other float is taken as
 * given: NaN, Inf and denormals go through the rules.  Generate touches region, heightmap, ridgemap, height_edit; derive region, heightmap,
 * ridgemap, normalmap, splatmap, splat_edit; minmax region, heightmap, patch_minmax.
 * One launch per stage; no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
#define OXC_TERRAIN_GENERATE 1u
#define OXC_TERRAIN_DERIVE 2u
#define OXC_TERRAIN_MINMAX 4u
typedef struct oxc_terrain_erosion { /* GPU::TerrainErosion (SceneGPU.hpp:358-372, scene.slang:541-558) */
  float scale, strength, gully_weight, detail;
  float rounding[4];
  float onset[4];
  float assumed_slope[2];
  float cell_scale, gain, lacunarity, normalization;
  uint32_t octaves, seed;
} oxc_terrain_erosion;
typedef struct oxc_terrain_generate { /* GPU::TerrainGenerate (SceneGPU.hpp:374-384) */
  oxc_terrain_erosion erosion;
  uint32_t resolution[2];
  float height_offset[2];
  float domain_size, height_frequency, height_amplitude, height_lacunarity, height_gain;
  uint32_t height_octaves;
} oxc_terrain_generate;
typedef struct oxc_terrain_derive { /* GPU::TerrainDerive (SceneGPU.hpp:386-395); the caller fills the first three as Terrain::bake does */
  uint32_t resolution[2];
  float texel_world_size[2]; /* world_size / resolution */
  float height_range;        /* height_range.y - height_range.x */
  float slope_rock_begin, slope_rock_end, altitude_snow_begin, altitude_snow_end, ridge_drainage_scale;
} oxc_terrain_derive;
#ifdef __cplusplus
static_assert(sizeof(oxc_terrain_erosion) == 80 && sizeof(oxc_terrain_generate) == 120 && sizeof(oxc_terrain_derive) == 40, "the GPU:: records");
#else
_Static_assert(sizeof(oxc_terrain_erosion) == 80 && sizeof(oxc_terrain_generate) == 120 && sizeof(oxc_terrain_derive) == 40, "the GPU:: records");
#endif
typedef struct oxc_terrain_maps_context {
  uint32_t struct_size; /* sizeof(oxc_terrain_maps_context) */
  uint32_t stages;      /* OXC_TERRAIN_GENERATE | OXC_TERRAIN_DERIVE | OXC_TERRAIN_MINMAX */
  oxc_terrain_generate generate;
  oxc_terrain_derive derive;
  uint32_t resolution[2], patch_count[2];              /* GPU::TerrainMinMax */
  uint32_t dispatch_texels[2], dispatch_patches[2];    /* the reference's dispatch arguments: bake passes resolution and patch_count */
  oxc_buffer region;       /* in, device memory, may be null: u32[4] {texel_origin.xy, patch_origin.xy} */
  oxc_buffer heightmap;    /* u16 [resolution.y][.x]: written by generate, read by derive and minmax */
  oxc_buffer ridgemap;     /* u16 [resolution.y][.x] of binary16 bits: written by generate, read by derive */
  oxc_buffer normalmap;    /* out (derive): u16x2 [resolution.y][.x] */
  oxc_buffer splatmap;     /* out (derive): u32 [resolution.y][.x] */
  oxc_buffer height_edit;  /* in (generate): f32 [resolution.y][.x] */
  oxc_buffer splat_edit;   /* in (derive): u32 [resolution.y][.x] */
  oxc_image patch_minmax;  /* out (minmax): RG32F, one level, patch_count.x x patch_count.y */
} oxc_terrain_maps_context;

oxc_status oxc_generate_terrain_maps(oxc_ctx* ctx, const oxc_terrain_maps_context* context, void* hip_stream);

/* ---- the terrain brush: the mouse ray against the heightmap, and the strokes into the edit images -------------------------------------------
 * oxc_apply_terrain_brush is the two compute passes of RendererInstance::apply_terrain_brush (Passes/Terrain.cpp:35-132):
 * passes/terrain_brush_trace.slang and passes/terrain_brush_apply.slang with GPU::TerrainBrushParams (scene.slang:606-630).  Trace marches
 * the ray through the heightmap and writes `hit` and `region`, the record oxc_generate_terrain_maps reads on the device; apply reads `hit`
 * from the device and writes the brush footprint into height_edit (modes Raise, Smooth, Flatten, Noise) or splat_edit (PaintLayer).  `stages`
 * selects them; the selected ones run in the order trace, apply on the stream.  Apply alone works on a hit written earlier: the reference's
 * `painting == false` split seen from the other side.  Images, formats and the arithmetic conventions are those of the terrain maps block:
 * binary32, the Slang's expressions left to right, one rounding per operation, no contraction; min / max / clamp / saturate through fmin /
 * fmax; the dots, length and normalize as defined there; the unorm8 and unorm16 load and store rules; decimal literals the nearest binary32
 * (1e-6f, 1e9f, 1e-3f, 0.05f).  Stated deviation: every float-to-integer conversion is cvt_u32_sat / cvt_i32_sat (saturating, a NaN gives 0)
 * where the Slang's conversion of a NaN or an out-of-range value is undefined.  B = params (oxc_terrain_brush_params).
 *   B1. the ray   direction = normalize(B.ray_direction) (a zero direction gives NaN in every component).  world_to_uv(w) = (w - B.world_min)
 *              * B.inv_world_size;  decode_height(n) = B.base_height + n * B.height_scale.
 *   B2. clip_to_footprint   world_max = B.world_min + B.world_size;  near = 0, far = 1e9f;  for the axes (origin.x, direction.x, world_min.x,
 *              world_max.x) and then (origin.z, direction.z, world_min.y, world_max.y) as (o, d, lo, hi):  if |d| < 1e-6f: if o < lo || o >
 *              hi the span is (1, 0) at once, else the axis is skipped;  otherwise t0 = (lo - o) / d, t1 = (hi - o) / d, near = max(near,
 *              min(t0, t1)), far = min(far, max(t0, t1)).  span = (near, far).  span.x <= span.y false (a NaN included) is a miss.
 *   B3. sample_height(w)   uv = world_to_uv(w).  Stated rule: SampleLevel(LinearSamplerClamped, uv, 0) is the manual bilinear of the
 *              oxc_apply_bloom block in clamp mode on the resolution.x x resolution.y heightmap, applied to the unorm16 loads: per axis g = uv
 *              * f32(resolution) - 0.5f, i = cvt_i32_sat(floor(g)), f = g - floor(g), the texels i and i + 1 each clamped to [0, resolution -
 *              1];  n = lerp(lerp(t00, t10, f.x), lerp(t01, t11, f.x), f.y);  sample_height = decode_height(n).
 *   B4. march   step = (span.y - span.x) / 512.0f;  t_0 = span.x exactly, t_i = span.x + step * f32(i) for i = 1 .. 512;  position_i =
 *              B.ray_origin + direction * t_i per component;  gap_i = position_i.y - sample_height(position_i.xz) (the Slang's i = 0 gap,
 *              ray_origin.y + direction.y * t, is the same expression).  The crossing is the smallest i in 1 .. 512 with gap_i <= 0 &&
 *              gap_(i-1) > 0; a NaN makes both comparisons false.  No gap depends on an earlier one.  Without a crossing: a miss.
 *   B5. bisect   lo = t_(i-1), hi = t_i;  24 times: mid = (lo + hi) * 0.5f, gap at mid as in B4;  gap > 0 ? lo = mid : hi = mid (a NaN takes
 *              hi).  world_position = B.ray_origin + direction * hi;  hit = {world_position, 1}.
 *   B6. region   center_texel = world_to_uv(world_position.xz) * f32(B.resolution);  radius = B.radius_texels + 1.0f;  texel_origin =
 *              cvt_u32_sat(max(floor(center_texel - radius), 0)) per component (max through fmax: a NaN gives 0);  patch_scale =
 *              f32(B.patch_count) / f32(B.resolution);  patch_origin = cvt_u32_sat(max(floor((center_texel - radius) * patch_scale), 0)).
 *              Trace always writes all 32 bytes of hit and region; on a miss it writes zeros.
 *   B7. apply, the texel   hit.valid == 0 writes nothing.  center = world_to_uv(hit.world_position.xz) * f32(B.resolution);  radius =
 *              cvt_i32_sat(ceil(B.radius_texels));  signed_texel = cvt_i32_sat(floor(center)) - radius + thread per component, evaluated
 *              without wrapping (a 64-bit sum; stated deviation: the Slang's i32 sum wraps);  a component below 0 or at least
 *              B.resolution writes nothing, so a centre far outside the map writes nothing.  The grid is sized on the host from
 *              radius_texels alone: footprint = 2 * u32(ceil(radius_texels)) + 1 threads a side in whole 16 x 16 groups, the reference's
 *              dispatch.
 *   B8. falloff   radius_texels <= 0 gives 0.  distance = length((f32(texel) + 0.5f) - center);  t = saturate(1.0f - distance /
 *              B.radius_texels);  smoothed = ((t * t) * t) * (t * (t * 6.0f - 15.0f) + 10.0f);  falloff = pow(smoothed, max(B.falloff,
 *              1e-3f)), pow the pow rule of oxc_apply_pbr: a base that is zero, below 2^-126, negative or NaN gives 0.  falloff <= 0 writes
 *              nothing.  amount = falloff * B.strength.
 *   B9. PaintLayer (mode 4)   target = (layer == 1 ? 1 : 0, layer == 2 ? 1 : 0, layer == 3 ? 1 : 0, 1): a layer outside 1 .. 3 paints (0, 0,
 *              0, 1).  splat_edit[texel] = the unorm8 stores of lerp(p, target, saturate(amount)) per component, p the four unorm8 loads of
 *              splat_edit[texel], lerp(a, b, t) = a + (b - a) * t.
 *   B10. the height modes   load_height(c) = the unorm16 load of the heightmap at c clamped to [0, resolution - 1] per axis;  height =
 *              load_height(texel).  Raise (0): delta = amount.  Smooth (1): sum = 0 and then sum = sum + load_height(texel + (x, y)) for y
 *              in -2 .. 2 and inside it x in -2 .. 2; delta = (sum / 25.0f - height) * amount.  Flatten (2): delta = (B.flatten_height -
 *              height) * amount.  Noise (3): delta = noised(f32(texel) * 0.05f, 0).x * amount, noised step T3 with seed 0.
 *              height_edit[texel] = clamp(height_edit[texel] + delta, -1, 1) (a NaN gives -1).
 * A texel is written by at most one thread; Smooth reads the heightmap, never height_edit, so there is no ordering between threads to
 * define.  Every byte the rule does not write stays as it was.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its own):
 * struct_size; stages non-zero with no unknown bit; every side of resolution in 1 .. 16384; every side of patch_count in 1 .. 4096; mode in
 * 0 .. 4; radius_texels finite and in 0 .. 4096 (this limit is the library's: it bounds the apply grid at 513 x 513 groups); falloff finite,
 * the pow rule's domain; every buffer a requested stage touches, in the order of the context's fields, non-null, then aligned to its texel
 * (hit and region to 8 bytes), then at least as large as its extent; no written buffer shares a byte with another buffer the requested
 * stages touch.  Trace touches heightmap, hit, region; apply in modes 0 - 3 heightmap, height_edit, hit; apply in PaintLayer splat_edit,
 * hit.  Every other float goes through the rules as given: NaN / Inf rays, a zero direction, a zero world_size, a NaN strength.
 * One launch per stage; no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
#define OXC_TERRAIN_BRUSH_TRACE 1u
#define OXC_TERRAIN_BRUSH_APPLY 2u
#define OXC_TERRAIN_BRUSH_RAISE 0u /* GPU::TerrainBrushMode (scene.slang:593-599) */
#define OXC_TERRAIN_BRUSH_SMOOTH 1u
#define OXC_TERRAIN_BRUSH_FLATTEN 2u
#define OXC_TERRAIN_BRUSH_NOISE 3u
#define OXC_TERRAIN_BRUSH_PAINT_LAYER 4u
typedef struct oxc_terrain_brush_params { /* GPU::TerrainBrushParams (scene.slang:606-621), field for field */
  float ray_origin[3], radius_texels;
  float ray_direction[3], strength;
  uint32_t resolution[2];
  float world_min[2], world_size[2], inv_world_size[2];
  uint32_t patch_count[2];
  float base_height, height_scale, falloff, flatten_height;
  uint32_t mode, layer;
} oxc_terrain_brush_params;
typedef struct oxc_terrain_brush_hit { /* GPU::TerrainBrushHit (scene.slang:601-604) */
  float world_position[3];
  uint32_t valid;
} oxc_terrain_brush_hit;
typedef struct oxc_terrain_region { /* GPU::TerrainRegion (scene.slang:588-591): what oxc_terrain_maps_context.region points at */
  uint32_t texel_origin[2], patch_origin[2];
} oxc_terrain_region;
#ifdef __cplusplus
static_assert(sizeof(oxc_terrain_brush_params) == 96 && sizeof(oxc_terrain_brush_hit) == 16 && sizeof(oxc_terrain_region) == 16, "the GPU:: records");
#else
_Static_assert(sizeof(oxc_terrain_brush_params) == 96 && sizeof(oxc_terrain_brush_hit) == 16 && sizeof(oxc_terrain_region) == 16, "the GPU:: records");
#endif
typedef struct oxc_terrain_brush_context {
  uint32_t struct_size; /* sizeof(oxc_terrain_brush_context) */
  uint32_t stages;      /* OXC_TERRAIN_BRUSH_TRACE | OXC_TERRAIN_BRUSH_APPLY */
  oxc_terrain_brush_params params;
  oxc_buffer heightmap;   /* in: u16 [resolution.y][.x], R16 Unorm */
  oxc_buffer height_edit; /* in/out (apply, modes 0 - 3): f32 [resolution.y][.x] */
  oxc_buffer splat_edit;  /* in/out (apply, PaintLayer): u32 [resolution.y][.x], R8G8B8A8 Unorm */
  oxc_buffer hit;         /* device memory, 16 bytes of oxc_terrain_brush_hit: written by trace, read by apply */
  oxc_buffer region;      /* device memory, 16 bytes of oxc_terrain_region: written by trace */
} oxc_terrain_brush_context;

oxc_status oxc_apply_terrain_brush(oxc_ctx* ctx, const oxc_terrain_brush_context* context, void* hip_stream);

/* ---- the terrain decode: the G-buffer images of the terrain pixels --------------------------------------------------------------------------
 * oxc_decode_terrain is RendererInstance::decode_terrain (Passes/Terrain.cpp:279-360, pipeline terrain_decode, passes/terrain_decode.slang),
 * the full-screen pass directly after decode_visbuffer (RendererInstance.cpp:929-952): per terrain pixel the world position is unprojected
 * from the depth, the normal map and the splat map are sampled there, the four splat layers are blended by weight, the brush ring is drawn,
 * and the four G-buffer images oxc_decode_visbuffer writes for the mesh pixels are written for the ground.  It runs after
 * oxc_decode_visbuffer on the same attachments.  The first consumer of the normal map and the splat map of oxc_generate_terrain_maps and of
 * the `hit` record of oxc_apply_terrain_brush.
 * Scope: the cut of oxc_decode_visbuffer -- the geometry and material-factor half of the shader; texture sampling is NOT done (D6).  The
 * tessellated terrain draw (terrain_visbuffer.slang) that produces the terrain texels and their depth is oxc_draw_terrain below.
 * Arithmetic: the conventions of the terrain maps block (binary32, the Slang's expressions left to right, one rounding per operation, no
 * contraction; min / max / saturate through fmin / fmax, so saturate(NaN) = 0; length, normalize, lerp(a, b, t) = a + (b - a) * t and
 * smoothstep as oxc_apply_pbr states them; the unorm8 load f32(byte) / 255.0f; a binary16 load is exact, denormals kept); decimal literals
 * the nearest binary32 (1e-4f, 0.02f, 0.05f, 0.55f, 0.1f); a comparison with a NaN operand is false.  T = terrain (oxc_terrain_data).
 * Per pixel (x, y) of the W x H images:
 *   D1. selection  (terrain_decode.slang:179-182)  A pixel whose visbuffer texel is not is_terrain ((texel >> 8) == 0xFFFFFE,
 *              visbuffer.slang:16-20) is not touched: the Slang's discard.  There is no clear flag; mesh texels, ~0u and every other texel
 *              keep the bytes the earlier passes left in all four images.  The depth texel's bits play no part in the selection: a terrain
 *              texel over depth 0 is decoded by the rule.
 *   D2. position   (:80-81)  uv = ((f32(x) + 0.5) / f32(W), (f32(y) + 0.5) / f32(H)).  Stated rule: the Slang's u32x2(uv * camera.resolution)
 *              with resolution == (W, H) is (x, y): the depth is the load of texel (x, y).  world = Camera::unproject_uv(uv, depth)
 *              (scene.slang:189-193): h = mul(inv_projection_view, (uv * 2.0 - 1.0, depth, 1)) row by row, ((m0 a + m1 b) + m2 c) + m3 as in
 *              oxc_apply_pbr step 3;  world = h.xyz / h.w, three divisions.  A depth of 0 or a zero h.w runs on with the IEEE results.
 *   D3. geometric normal  (:84-86)  terrain_uv = (world.xz - T.world_min) * T.inv_world_size.  SampleLevel(LinearSamplerClamped, terrain_uv, 0)
 *              on the normal map and on the splat map is the manual clamp bilinear of oxc_apply_terrain_brush step B3 on the
 *              map_resolution.x x map_resolution.y maps, applied per channel to the two binary16 loads of a normal-map texel and to the
 *              four unorm8 loads of a splat-map texel: n = (normal map .x, .y), w = the four splat channels.  geometric_normal =
 *              normalize((n.x, sqrt(saturate(1.0 - (n.x * n.x + n.y * n.y))), n.y)): dot(n, n) > 1 gives a zero y, a NaN in n a NaN normal.
 *   D4. weights    (:105-107)  weight_sum = ((w.x + w.y) + w.z) + w.w;  weights = weight_sum > 1e-4f ? w / weight_sum (four divisions) :
 *              (1, 0, 0, 0).  A NaN weight_sum takes the second arm.
 *   D5. layers     (:38-77)  albedo (four channels), emissive, metallic, roughness and occlusion start at 0.  For i = 0 .. 3 in order, weight =
 *              weights[i]:  weight <= 0 skips the layer (a NaN weight does not).  index = T.layer_material_indices[i].  index ==
 *              TERRAIN_INVALID_LAYER_MATERIAL (~0u, scene.slang:632): albedo += (1, 1, 1, 1) * weight, (metallic, roughness) += (0.0, 1.0) *
 *              weight (the product 0.0 * weight is formed), occlusion += weight, nothing is added to emissive.  Any other index >=
 *              material_count uses the all-zero Material of oxc_decode_visbuffer; otherwise the record materials_buffer[index].  Its
 *              factors -- the four halves of albedo_color, the three of emissive_color, metallic_factor, roughness_factor -- go through the
 *              flushing com::dequantize_half (oxc_decode_visbuffer step 3) and each sum is sum = sum + factor * weight; occlusion += 1.0 *
 *              weight.  Sums accumulate in layer order.
 *   D6. out of scope, stated  Texture sampling is not done: the Has*Image and NormalFlipY bits are ignored and every sample_* returns its
 *              factor alone, as in oxc_decode_visbuffer.  Nothing that only feeds a SampleGrad is computed: the two neighbour rays with
 *              plane_offset, ddx_world and ddy_world (:88-103), inv_tiling (:109), the side projection's uv and gradients (:120-123);
 *              T.layer_tiling and Camera::position are not read.  Consequences: (a) the side sample (:125-127) reads the same factors with
 *              the same weights as the top sample, so the triplanar blend (:110-111, 119-139) is dropped and with it slope and
 *              triplanar_amount; T.triplanar_begin is not read.  lerp(a, a, t) is a for every finite a and t; stated deviation: a
 *              non-finite sum (an Inf or NaN factor, a NaN weight) is stored as D5 left it, where the Slang's a + (a - a) * t would turn
 *              an Inf into a NaN on slopes with triplanar_amount > 0, and a NaN triplanar_amount is not spread into finite sums.  (b)
 *              every layer's tangent normal is (0, 0, 1), the blended one normalises to (0, 0, 1) or takes the (0, 0, 1) fallback, and the
 *              tangent frame (:116-149) multiplies zeros: shading_normal = normalize(geometric_normal), the second normalisation kept
 *              because the Slang performs it (:154-156).  A zero weight total, which leaves the blended tangent normal at its fallback, gives
 *              the same.
 *   D7. brush ring (:158-164)  Only when T.brush_radius > 0 (false for a NaN) and hit.valid != 0; hit is read from device memory, and not
 *              read at all unless T.brush_radius > 0.  d = world.xz - hit.world_position.xz;  ring_distance = sqrt(d.x * d.x + d.y * d.y);
 *              ring_width = max(T.brush_radius * 0.02f, 0.05f);  ring = 1.0 - smoothstep(0.0, ring_width, |ring_distance -
 *              T.brush_radius|);  albedo.rgb = lerp(albedo.rgb, (1.0, 0.55f, 0.1f), ring) per channel; alpha is left.
 *   D8. stores     albedo_attachment: r, g, b through the sRGB encoding and every channel through the unorm8 rule, alpha linear
 *              (oxc_decode_visbuffer step 6).  normal_attachment: .rg = vec3_to_oct(shading_normal), .ba = vec3_to_oct(geometric_normal),
 *              four binary16 by step 5 there (a NaN stored as 0x7E00).  emissive_attachment: B10G11R11 by the UF11 / UF11 / UF10 rule of
 *              step 8.  metallic_roughness_occlusion_attachment: (metallic, roughness, occlusion, 0.0) by the unorm8 rule, metallic in the
 *              low byte (step 7).
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its own):
 * struct_size; width and height non-zero; both equal to the depth attachment's, which is one R32F level at offset 0 of at most 65536 a
 * side; every side of map_resolution in 1 .. 16384; then every buffer in the order of the context's fields -- visbuffer_attachment,
 * depth_attachment, normalmap, splatmap, materials_buffer, brush_hit and the four outputs -- non-null, then aligned to its texel (4 bytes; the
 * normal attachment and brush_hit 8), then at least as large as its extent (one texel per pixel or per map texel; material_count records
 * of 56 bytes; 16 bytes of brush_hit); materials_buffer may be null when material_count is 0 and brush_hit when T.brush_radius > 0 is false
 * (a buffer that may be null and is null is not checked further and not read); then no output shares a byte with any other buffer of the
 * call.  Every float is taken as given: NaN / Inf in the matrix, in world_min, inv_world_size and brush_radius run through the rules.  The
 * layer indices need no limit (D5).  One launch, no scratch, no allocation, no host synchronisation; capturable into a HIP graph. */
#define OXC_TERRAIN_INVALID_LAYER_MATERIAL 0xFFFFFFFFu /* scene.slang:632 */
typedef struct oxc_terrain_data { /* GPU::TerrainData (scene.slang:634-661 with its world_to_uv, SceneGPU.hpp:440-453), field for field, 76 bytes */
  float world_min[2], world_size[2], inv_world_size[2];
  uint32_t patch_count[2];
  float base_height, height_scale, target_edge_pixels, max_tessellation, layer_tiling, triplanar_begin;
  uint32_t layer_material_indices[4];
  float brush_radius;
} oxc_terrain_data;
#ifdef __cplusplus
static_assert(sizeof(oxc_terrain_data) == 76, "GPU::TerrainData");
#else
_Static_assert(sizeof(oxc_terrain_data) == 76, "GPU::TerrainData");
#endif
typedef struct oxc_terrain_decode_context {
  uint32_t struct_size; /* sizeof(oxc_terrain_decode_context) */
  uint32_t width, height;
  float inv_projection_view[16]; /* Camera::inv_projection_view, column-major */
  oxc_terrain_data terrain;      /* read: world_min, inv_world_size, layer_material_indices, brush_radius */
  uint32_t map_resolution[2];    /* the extent of normalmap and splatmap */
  uint32_t material_count;
  oxc_buffer visbuffer_attachment; /* in: u32[height][width] */
  oxc_image depth_attachment;      /* in: R32F, levels = 1 */
  oxc_buffer normalmap;            /* in: u16x2 [map_resolution.y][.x], R16G16 Sfloat, as oxc_generate_terrain_maps writes it */
  oxc_buffer splatmap;             /* in: u32 [map_resolution.y][.x], R8G8B8A8 Unorm */
  oxc_buffer materials_buffer;     /* in: GPU::Material[material_count], 56 bytes each */
  oxc_buffer brush_hit;            /* in: device memory, 16 bytes of oxc_terrain_brush_hit, as oxc_apply_terrain_brush writes it */
  oxc_buffer albedo_attachment;    /* out, terrain pixels only: the four attachments of oxc_decode_context, same formats and layouts */
  oxc_buffer normal_attachment;
  oxc_buffer emissive_attachment;
  oxc_buffer metallic_roughness_occlusion_attachment;
} oxc_terrain_decode_context;

oxc_status oxc_decode_terrain(oxc_ctx* ctx, const oxc_terrain_decode_context* context, void* hip_stream);

/* ---- the terrain draw: tessellated patches into the depth|vis image ---------------------------------------------------------------------------
 * oxc_draw_terrain is RendererInstance::draw_terrain_for_visbuffer (Passes/Terrain.cpp:218-277, pipeline terrain_visbuffer,
 * passes/terrain_visbuffer.slang): the consumer of oxc_cull_terrain's visible_patches and VkDrawIndirectCommand {4, instance_count, 0, 0} and
 * the producer of the terrain texels oxc_decode_terrain reads.  It writes the u64 image of oxc_draw_visbuffer, so terrain and meshes compete
 * per pixel; with it a frame with ground runs cull -> draw -> HiZ -> late cull -> decode -> PBR on the device
 * (RendererInstance.cpp:868-884).  The reference's vertex positions come from the fixed-function tessellator, whose placement of the
 * fractional-odd short segments and triangulation of the outer ring the Vulkan specification leaves open; as with the rasteriser, the rules
 * are stated here (T1 - T7), implemented twice (tests/terrain_draw_model.py and the device code) and held to byte identity, and a stated
 * rule is one of the behaviours the reference may legally show.
 * Arithmetic: the conventions of the terrain maps block -- binary32, the Slang's expressions left to right, one rounding per operation, no
 * contraction; lerp(a, b, t) = a + (b - a) * t; distance(a, b) = sqrt((dx * dx + dy * dy) + dz * dz) of d = a - b, IEEE sqrt; min / max /
 * clamp through fminf / fmaxf (a NaN operand loses); IEEE division.  T = terrain (oxc_terrain_data).
 *   T1. corners   (vs_main)  instance_count = draw_cmd[1] and first_instance = draw_cmd[3] are read on the device; words 0 and 2 are not
 *              read.  For i in 0 .. instance_count - 1: p = visible_patches[first_instance + i] (the sum in 64 bits).  An entry at or past
 *              the end of visible_patches_buffer (or past its first 2^24 entries, more than any grid has patches), or p >= T.patch_count.x * T.patch_count.y, is skipped and counted (the Slang would run
 *              on garbage).  patch = (p % T.patch_count.x, p / T.patch_count.x).  Corner c of (0,0), (1,0), (1,1), (0,1) named p0 .. p3:
 *              grid = f32(patch + c) / f32(T.patch_count) per component;  xz = T.world_min + grid * T.world_size (scene.slang:649-652):
 *              neighbouring patches form the same integers, so a shared corner has the same bits.  y = sample_height(xz), step B3 of
 *              oxc_apply_terrain_brush on the map_resolution.x x map_resolution.y heightmap with T's world_min, inv_world_size, base_height
 *              and height_scale.  world = (xz.x, y, xz.y).
 *   T2. factors   (edge_tessellation, hs_constants)  For an edge (a, b): center = (a + b) * 0.5 per component;  radius = distance(a, b) *
 *              0.5;  view_distance = max(distance(center, camera_position) - radius, near_clip);  projected_pixels = ((2.0 * radius) *
 *              projection_scale) / view_distance;  factor = clamp(projected_pixels / T.target_edge_pixels, 1.0, T.max_tessellation) =
 *              fminf(fmaxf(q, 1.0), max_tessellation).  projection_scale is taken as given: the engine's value is resolution.y * 0.5 /
 *              tan(radians(fov) * 0.5); the bindings have a helper that evaluates it in binary64 and rounds once, so no transcendental
 *              enters the rule.  Edges 0: (p0, p3), 1: (p0, p1), 2: (p1, p2), 3: (p3, p2).  inside[0] = max(e1, e3) subdivides u;
 *              inside[1] = max(e0, e2) subdivides v.  A patch with any edge factor <= 0 or NaN is discarded and counted (Vulkan's rule;
 *              reachable with max_tessellation <= 0, or a NaN from the camera or the maps).
 *   T3. fractional_odd subdivision of one factor f   fc = fminf(fmaxf(f, 1), 63);  n = the smallest odd integer >= fc;  r = 1.0f / fc;
 *              s = (1.0f - f32(n - 2) * r) * 0.5f;  t_0 = 0, t_n = 1;  t_k = s + f32(k - 1) * r for 1 <= k <= (n - 1) / 2;  t_k = 1.0f -
 *              t_(n-k) above that.  n == 1 gives {0, 1}.  That is n - 2 segments of length 1 / f and two shorter ones at the ends, which
 *              shrink to nothing as f falls to n - 2.
 *   T4. topology  (the Vulkan quad rule)  If all six n are 1 the patch is the two triangles (p0, p1, p2), (p0, p2, p3) in (u, v).
 *              Otherwise an inner n of 1 is redone with fc = 0x3F800001 (n = 3), U = the inside[0] list (nu segments), V = the inside[1]
 *              list (nv), and the patch is: the inner grid (U_i, V_j), 1 <= i <= nu - 1, 1 <= j <= nv - 1, every cell as ((i, j), (i+1, j),
 *              (i+1, j+1)) and ((i, j), (i+1, j+1), (i, j+1));  and four ring strips -- side 0: outer points (0, t) over edge 0's list
 *              against the inner points (U_1, V_j); side 1: (t, 0) over edge 1's list against (U_i, V_1); side 2: (1, t) over edge 2's
 *              against (U_(nu-1), V_j); side 3: (t, 1) over edge 3's against (U_i, V_(nv-1)).  A strip is the merge of its two sorted
 *              parameter lists from (outer 0, inner 1): advance the outer point when the inner list is exhausted, or when the outer list
 *              is not exhausted and its next parameter <= the inner list's next parameter; otherwise advance the inner point.  The
 *              triangle is (current outer, current inner, the point advanced to); on sides 1 and 2 its last two corners are exchanged.
 *              With these orders every triangle of non-zero area is counter-clockwise in (u, v).  Triangles per patch: 2 (nu - 2)(nv - 2)
 *              + sum over the sides of (n_side + n_inner_axis - 2), at most 7938.
 *   T5. domain point  (ds_main)  a = lerp(p0, p1, u), b = lerp(p3, p2, u), q = lerp(a, b, v) on x and z;  world = (q.x,
 *              sample_height(q.xz), q.z);  clip = mul(projection_view, (world, 1)) row by row, ((m0 x + m1 y) + m2 z) + m3, as
 *              oxc_decode_visbuffer step 4.  Stated deviation: a lerp whose coordinate is exactly 0 or 1 returns its first or second operand
 *              itself (the Slang's a + (b - a) * 1 can differ from b in the last bit).  With it the points of an edge two patches share
 *              are bit-identical from both, and the top-left rule makes the seam watertight.  A point is evaluated once.
 *   T6. facing    A triangle seen from +y is a front face: a triangle (c0, c1, c2) of T4 is handed to the set-up as (c0, c2, c1), the one
 *              global exchange under which cullMode eBack of oxc_draw_visbuffer (fixed-point area >= 0 is dropped) keeps the triangles
 *              a camera above the ground sees.  (DESIGN.md section 30 derives what the reference's state gives.)
 *   T7. raster    The oxc_draw_visbuffer block unchanged on the three clip-space corners in T6's order: the clipper against the five
 *              planes with its fan, set-up, cover, depth in (0, 1], with vis = 0xFFFFFE00 (VisBufferData(TERRAIN_INSTANCE_ID, 0).encode())
 *              and the 64-bit maximum of depth bits << 32 | vis.  Terrain therefore wins an exact depth tie against every mesh texel: what
 *              GreaterOrEqual with the terrain drawn second gives.
 * `clear` zeroes the image first; without it the call adds to what oxc_draw_visbuffer or an earlier call left.  The optional resolves are
 * those of oxc_draw_visbuffer (vis 0 / depth 0 for uncovered pixels).
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its own):
 * struct_size; width and height in 1 .. 16384; every side of map_resolution in 1 .. 16384; every side of terrain.patch_count in 1 .. 4096;
 * then the buffers in the order heightmap, visible_patches_buffer, draw_cmd_buffer, visdepth_buffer -- non-null, then aligned to its texel
 * (2, 4, 4 and 8 bytes), then at least as large as its extent (map texels of 2 bytes; one u32; 16 bytes; width * height u64);
 * depth_attachment, when given, one R32F level of the draw's extent; visbuffer_attachment, when given, width * height u32.  Every float is
 * taken as given.  The scratch (big list, tiles) is the one oxc_draw_visbuffer uses, allocated by whichever of the two draws runs first on
 * the context: that first call must not be captured; afterwards the call allocates nothing, does not synchronise the host and is
 * capturable into a HIP graph. */
typedef struct oxc_terrain_draw_context {
  uint32_t struct_size; /* sizeof(oxc_terrain_draw_context) */
  uint32_t clear;
  uint32_t width, height;
  float projection_view[16]; /* Camera::projection_view, column-major */
  float camera_position[3];
  float near_clip;
  float projection_scale;        /* T2 */
  oxc_terrain_data terrain;      /* read: world_min, world_size, inv_world_size, patch_count, base_height, height_scale, target_edge_pixels, max_tessellation */
  uint32_t map_resolution[2];    /* the extent of heightmap */
  oxc_buffer heightmap;              /* in: u16 [map_resolution.y][.x], R16 Unorm, as oxc_generate_terrain_maps writes it */
  oxc_buffer visible_patches_buffer; /* in: u32 patch indices, as oxc_cull_terrain writes them */
  oxc_buffer draw_cmd_buffer;        /* in: VkDrawIndirectCommand {vertex_count, instance_count, first_vertex, first_instance}, read on the device */
  oxc_buffer visdepth_buffer;        /* in/out: u64[height][width], the image of oxc_draw_visbuffer */
  oxc_image depth_attachment;        /* optional resolve: R32F */
  oxc_buffer visbuffer_attachment;   /* optional resolve: u32[height][width] */
} oxc_terrain_draw_context;

oxc_status oxc_draw_terrain(oxc_ctx* ctx, const oxc_terrain_draw_context* context, void* hip_stream);

/* ---- the debug views: what the cull, the LOD select, the rasteriser, the decodes and the page update decided, as a picture ----------------
 * oxc_apply_debug_view is RendererInstance::apply_debug_view (Passes/Debug.cpp:9-153, pipelines debug_view and rmvsm_debug, shaders
 * passes/debug_view.slang and passes/rmvsm_debug.slang), the pass that replaces the final image when a debug view is selected
 * (RendererInstance.cpp:1300-1323): per pixel a colour for the triangle, meshlet, material, mesh or LOD behind the visbuffer texel, the
 * overdraw heat, one G-buffer channel or the ambient occlusion, with a depth outline; or, for OXC_DEBUG_VIEW_RMVSM, the state of the VSM
 * page the pixel falls in.  One launch, one R16G16B16A16 Sfloat image out.
 * Not built: a producer for the overdraw image (oxc_draw_visbuffer has no counting mode, visbuffer_encode.slang:69-71; the caller fills
 * the u32 image); draw_bounding_boxes (Debug.cpp:155-211, line rasterisation).  The editor's picking and highlight passes are
 * oxc_pick_transform and oxc_apply_highlight below.
 * Arithmetic: the conventions of oxc_apply_pbr's block -- binary32, round to nearest even, the Slang's order left to right, no
 * contraction, IEEE division; min, max and saturate through fminf / fmaxf (a NaN operand loses, saturate(NaN) = 0); a comparison with a
 * NaN operand is false; f32(u32) rounds to nearest even; a half store is round to nearest even with denormals kept and a NaN stored as
 * 0x7E00 (oxc_apply_pbr step 12); log2 is the log2 rule of oxc_generate_ambient_occlusion rounded to binary32 once (an argument below
 * 2^-126, negative or NaN gives -Inf), exp2 the exp2 rule of oxc_apply_pbr.  TAU = 6.283185307179586f, the nearest binary32.  The float
 * `%` is fmodf, which is exact; a non-finite operand gives NaN.
 *   hash(a)  (debug_view.slang:31-39), modulo 2^32:  a = (a + 0x7ed55d16) + (a << 12);  a = (a ^ 0xc761c23c) ^ (a >> 19);  a = (a +
 *              0x165667b1) + (a << 5);  a = (a + 0xd3a2646c) ^ (a << 9);  a = (a + 0xfd7046c5) + (a << 3);  a = (a ^ 0xb55a4f09) ^ (a >> 16).
 *              hash colour of h = hash(a): (f32(h & 255), f32((h >> 8) & 255), f32((h >> 16) & 255)) / 255.0f, three divisions.
 *   hsv_to_rgb((hue, 1.0, 0.5))  (:25-29, rmvsm_debug.slang:14-18)  q = hue / 1.0471975512f;  per component of n = (5.0, 3.0, 1.0):  k =
 *              fmodf(n + q, 6.0f);  0.5 - (0.5 * 1.0) * max(0.0, min(k, min(4.0 - k, 1.0))).  A NaN k gives 0.5 - 0.5 * 1.0 = 0.0.
 * The main views (debug_view.slang), per pixel (x, y) of the W x H images, texel = the visbuffer texel:
 *   V1. discard  (:97-101)  texel == ~0u: with `clear` the pixel is written as the four halves 0, 0, 0, 0x3C00, otherwise it is not
 *              touched.  Stated rule: that value stands for the engine's clear_image(.., vuk::Black) in front of the pass (Debug.cpp:34);
 *              the vuk header that defines Black is not part of the reference tree.
 *   V2. colour   (:109-164)
 *              Triangles: the hash colour of texel & 0xFF.  Meshlets: of texel >> 8.  Neither reads a record.
 *              Materials: of mesh_instance.material_index.  MeshInstances: of mesh_instance.mesh_index, as the Slang does despite the
 *              name.  mesh_instance = mesh_instances[meshlet_instances[texel >> 8].mesh_instance_index], by V3.
 *              MeshLods: hue = (f32(mesh_instance.lod_index) / f32(mesh.lod_count + 1)) * TAU, the u32 sum wrapping (lod_count ==
 *              0xFFFFFFFF divides by 0.0), mesh = meshes[mesh_instance.mesh_index];  hsv_to_rgb((hue, 1.0, 0.5)).
 *              Overdraw: draw_scale = min(max(heatmap_scale, 0.0), 100.0) / 100.0f (a NaN scale gives 0);  heat = 1.0 - exp2((-f32(count))
 *              * draw_scale), count the overdraw texel;  t = saturate(heat);  inferno(t) per channel = c0 + t * (c1 + t * (c2 + t * (c3 + t
 *              * (c4 + t * (c5 + t * c6))))) as nested at :51, the seven constants of :42-48 the nearest binary32.
 *              Albedo: stated rule, as oxc_apply_pbr step 2 for the clamped sampler: the linear repeat sampler at the pixel centre is the
 *              load of texel (x, y); bytes R, G, B through the sRGB decode of that step.
 *              Normal: oct_to_vec3(.rg of the normal texel) * 0.5 + 0.5 per channel, oct_to_vec3 as in oxc_resolve_shadowmap step 2 (one
 *              normalisation).  GeometricNormal: the same on .ba.
 *              Emissive: the exact UF11 / UF11 / UF10 decode of oxc_apply_pbr step 2 (it can give Inf and NaN; V4 saturates them).
 *              Metallic, Roughness, BakedOcclusion: byte 0, 1 or 2 of the texel as f32(byte) / 255.0f, in all three channels.
 *              GTAO: the ambient-occlusion half, binary16 -> binary32 exact with denormals kept, in all three channels.
 *   V3. bounds   Stated rule for Materials, MeshInstances and MeshLods: a texel with (texel >> 8) >= meshlet_instance_count uses an
 *              all-zero MeshInstance and an all-zero Mesh -- hash(0), or hue (0.0 / 1.0) * TAU -- and loads nothing; terrain texels
 *              (0xFFFFFE) are the common case.  The Slang reads past the buffer there.  Every other index of the chain
 *              (mesh_instance_index, mesh_index) is the scene's own and is not checked, as in oxc_decode_visbuffer.  Triangles, Meshlets,
 *              Overdraw and the G-buffer views perform no record load at all: the Slang's three loads (:105-107) are dead code for them.
 *   V4. outline  (:54-89)  gx = gy = 0.0.  For tap = 0 .. 8 in the order of sample_offset, (-1, 1) (0, 1) (1, 1) (-1, 0) (0, 0) (1, 0) (-1, -1)
 *              (0, -1) (1, -1):  p = (x, y) + offset.  A tap outside the image adds nothing (the robust loads give texel 0 and depth 0, and
 *              log2(1.0) * 10.0 = 0.0 changes no sum); a tap whose visbuffer texel is ~0u is skipped.  Otherwise s = log2(depth(p) + 1.0f) *
 *              10.0f;  gx = gx + f32(sobel_x[tap]) * s;  gy = gy + f32(sobel_y[tap]) * s, sobel_x = 1 0 -1 2 0 -2 1 0 -1, sobel_y = 1 2 1 0
 *              0 0 -1 -2 -1.  The product with a zero weight is formed: 0.0 * Inf is NaN.  (The Slang's three channels of x and of y are
 *              equal; one is kept.)  outline = fmaxf(|gx|, |gy|);  colour = saturate(colour * (1.0 - outline)) per channel;  the store is
 *              the four halves of (colour, 1.0), R lowest.  s is -Inf for depth <= -1 and for a NaN depth, +Inf for +Inf, never NaN.
 * The RMVSM view (rmvsm_debug.slang), per pixel; no outline, no discard, `clear` is ignored, every pixel is written:
 *   R1. sky      (:25-28)  depth == 0.0 stores (1, 1, 1, 1) (a NaN depth is not sky).
 *   R2. set-up   (:33-39)  uv, world and the clipmap index c exactly as oxc_resolve_shadowmap step 2.  flat_N (:30-31) is unused and not
 *              computed; the normal image is not read.  h = M_c (world, 1);  clip_uv = (h.xy / h.w + 1.0) * 0.5, as in that block's tap.
 *   R3. texel    (:45-48)  A component of clip_uv outside [0, 1], or NaN (stated: a NaN counts as outside, as the resolve does): the in-page
 *              texel is page_size - 1 on both axes, the Slang's com::mod(-1, page_size).  Otherwise in_page = int(floor(clip_uv *
 *              f32(physical_page_table_size))) % page_size per axis, in integers -- the Slang's physical extent, NOT the resolve's V =
 *              page_table_size * page_size: this pass draws the grid the reference draws.  near_border = any(in_page < 2) || any(in_page >
 *              page_size - 2).
 *   R4. border   (:51-55)  near_border stores hsv_to_rgb(((f32(c) / f32(clipmap_count + 1)) * TAU, 1.0, 0.5)) with alpha 1.0 and reads no
 *              page-table entry.
 *   R5. page     (:41-43, 57-62)  virt = int(floor(clip_uv * f32(page_table_size))) per axis;  entry = virtual_page_table[c][wrapped.y]
 *              [wrapped.x], wrapped = floor_mod(virt + page_offset, page_table_size) as in oxc_update_virtual_shadowmap.  virt is inside
 *              the table: clip_uv lies in [0, 1], so virt >= 0; and n * u rounds to n only for u == 1.0 (for u <= 1 - 2^-24 the product is
 *              at least half an ulp of n below n), where in_page is physical_page_table_size % page_size = 0 and R4 has taken the pixel
 *              (f32(physical_page_table_size) is exact up to 2^24; beyond it the kernel still loads nothing outside the table: a virt
 *              outside [0, n - 1] reads entry 0, the Slang's robust load at INVALID_COORDS).  With the flag bits of
 *              oxc_update_virtual_shadowmap (Visible 1, Dirty 2, Backed 4):  not Backed and Visible stores (1, 0, 0, 1);  otherwise
 *              (Backed, Dirty, Visible, 1) as 0.0 or 1.0.
 * Inputs: an input the selected view does not read is not read, not checked and may be null (as the images of oxc_apply_pbr whose flag
 * is clear).  Every view except RMVSM reads visbuffer_attachment and depth_attachment (V1, V4); Overdraw also overdraw_attachment;
 * Albedo albedo_attachment; Normal and GeometricNormal normal_attachment; Emissive emissive_attachment; Metallic, Roughness and
 * BakedOcclusion metallic_roughness_occlusion_attachment; GTAO ambient_occlusion_attachment; Materials, MeshInstances and MeshLods the
 * frame's meshlet_instances_buffer, mesh_instances_buffer and meshes_buffer (`frame` may be NULL for every other view).  RMVSM reads
 * depth_attachment, vsm_clipmaps_buffer and virtual_page_table only, with the eleven VSM and camera fields.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its
 * own): struct_size; debug_view in OXC_DEBUG_VIEW_TRIANGLES .. OXC_DEBUG_VIEW_RMVSM (0, the reference's None, is refused: the engine does
 * not run the pass then); width and height non-zero; both equal to the depth attachment's, which is one R32F level at offset 0 of at most
 * 65536 a side; for RMVSM the shape limits of oxc_resolve_shadowmap; for Materials, MeshInstances and MeshLods `frame` non-null; then
 * every buffer the view reads in the order of the context's fields, then the frame's three, then debug_attachment -- non-null, then
 * aligned to its texel or record (4 bytes; ambient_occlusion_attachment 2; normal_attachment, debug_attachment and meshes_buffer, whose
 * GPU::Mesh records hold 64-bit addresses, 8), then at least as large as its
 * extent (one texel per pixel; clipmap_count records of 76 bytes; clipmap_count * n * n entries; meshlet_instance_count records of 8
 * bytes; the other two frame buffers as given); then debug_attachment shares no byte with any buffer the view reads.  heatmap_scale and
 * every other float are taken as given, NaN included.  One launch, no scratch, no allocation, no host synchronisation; capturable into a
 * HIP graph. */
#define OXC_DEBUG_VIEW_TRIANGLES 1u /* GPU::DebugView, scene.slang:10-26 and SceneGPU.hpp:28-47; 0 is None */
#define OXC_DEBUG_VIEW_MESHLETS 2u
#define OXC_DEBUG_VIEW_OVERDRAW 3u
#define OXC_DEBUG_VIEW_MATERIALS 4u
#define OXC_DEBUG_VIEW_MESH_INSTANCES 5u
#define OXC_DEBUG_VIEW_MESH_LODS 6u
#define OXC_DEBUG_VIEW_ALBEDO 7u
#define OXC_DEBUG_VIEW_NORMAL 8u
#define OXC_DEBUG_VIEW_EMISSIVE 9u
#define OXC_DEBUG_VIEW_METALLIC 10u
#define OXC_DEBUG_VIEW_ROUGHNESS 11u
#define OXC_DEBUG_VIEW_BAKED_OCCLUSION 12u
#define OXC_DEBUG_VIEW_GTAO 13u
#define OXC_DEBUG_VIEW_GEOMETRIC_NORMAL 14u
#define OXC_DEBUG_VIEW_RMVSM 15u /* the C++ enum's member after GeometricNormal (SceneGPU.hpp:44); the Slang enum stops at 14 */
typedef struct oxc_debug_view_context {
  uint32_t struct_size; /* sizeof(oxc_debug_view_context) */
  uint32_t width, height;
  uint32_t debug_view;             /* OXC_DEBUG_VIEW_* */
  uint32_t clear;                  /* V1: discarded pixels are written as 0, 0, 0, 0x3C00 */
  float heatmap_scale;             /* Overdraw: DebugContext::overdraw_heatmap_scale */
  uint32_t meshlet_instance_count; /* V3 */
  /* RMVSM: the GPU::VSMContext and GPU::Camera fields the pass reads, as in oxc_shadow_resolve_context */
  int32_t page_size, page_table_size, physical_page_table_size, clipmap_count;
  float first_clipmap_width;
  float clipmap_selection_bias;
  float virtual_extent;
  float inv_projection_view[16];   /* column-major */
  float resolution[2];
  oxc_buffer visbuffer_attachment; /* in: u32[height][width] */
  oxc_image depth_attachment;      /* in: R32F, levels = 1 */
  oxc_buffer overdraw_attachment;  /* in: R32 Uint, u32[height][width] */
  oxc_buffer albedo_attachment;    /* in: the four attachments of oxc_decode_context, same formats and layouts */
  oxc_buffer normal_attachment;
  oxc_buffer emissive_attachment;
  oxc_buffer metallic_roughness_occlusion_attachment;
  oxc_buffer ambient_occlusion_attachment; /* in: binary16 as u16[height][width], as oxc_apply_pbr reads it */
  oxc_buffer vsm_clipmaps_buffer;  /* in: oxc_virtual_clipmap[clipmap_count] */
  oxc_buffer virtual_page_table;   /* in: u32 [clipmap_count][n][n] */
  oxc_buffer debug_attachment;     /* out: R16G16B16A16 Sfloat, u16x4[height][width], R in the lowest half */
} oxc_debug_view_context;

oxc_status oxc_apply_debug_view(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_debug_view_context* context, void* hip_stream);

/* ---- the editor's selection path: which entity is under the cursor, and the outline around the selected ones -------------------------------
 * oxc_pick_transform is the `mouse_picking` stage and oxc_apply_highlight the `highlight_mask` and `entity_highlighting` stages of the
 * reference's editor (OxylusEditor/src/Panels/ViewportPanel.cpp:1166-1556: mouse_picking_stages, highlight_mask_stage,
 * highlight_composite_stage; shaders editor/mouse_picking.slang, highlight_mask.slang, highlight_dilate_horizontal.slang and
 * highlight_composite.slang).  mouse_picking_2d.slang is oxc_pick_sprite, in the block of oxc_draw_sprites below.
 * Arithmetic: the conventions of oxc_apply_debug_view's block -- binary32, round to nearest even, the Slang's order, no contraction, IEEE
 * division; saturate through fminf / fmaxf (saturate(NaN) = 0); a comparison with a NaN operand is false; pow by the pow rule of
 * oxc_apply_pbr (a base that is zero, negative, below 2^-126 or NaN has log2 -Inf).
 *   P. transform of a texel  (mouse_picking.slang:21-35, highlight_mask.slang:18-30)
 *              texel == ~0u: ~0u.  (texel >> 8) == 0xFFFFFE, a terrain texel: terrain_transform_index.  Otherwise
 *              mesh_instances[meshlet_instances[texel >> 8].mesh_instance_index].transform_index.  Stated rule, V3 of oxc_apply_debug_view:
 *              a texel with (texel >> 8) >= meshlet_instance_count uses an all-zero MeshInstance and loads nothing, so its transform is 0;
 *              the Slang reads past the buffer there.  mesh_instance_index is the scene's own and is not checked.
 * oxc_pick_transform writes P of the texel (x, y) as one u32 to transform_id.  Limits (else OXC_INVALID_ARG, nothing launched, nothing
 * written; the first broken rule in this order gives the message, each has its own): struct_size; width and height non-zero and at most
 * 65536; x < width and y < height; `frame` non-null; then visbuffer_attachment, transform_id, the frame's meshlet_instances_buffer and
 * mesh_instances_buffer, each non-null, then 4-byte aligned, then large enough (one u32 per pixel; one u32; meshlet_instance_count records
 * of 8 bytes; mesh_instances_buffer as given); then transform_id shares no byte with any of them.  One launch, no scratch, no allocation,
 * no host synchronisation; capturable into a HIP graph.
 *
 * oxc_apply_highlight runs the stages of `stages`, the mask first.  The engine runs the mask after VisBufferEncode and the rest after
 * post-processing, so each stage can be called alone.
 * Stage OXC_HIGHLIGHT_MASK (highlight_mask.slang), per pixel (x, y):
 *   M1. selected  (:15-41)  t = P of the visbuffer texel.  Not selected when the texel is ~0u or t == ~0u; otherwise selected when t equals
 *              one of the selected_count entries of transform_indices that is not ~0u.  selected_count == 0 selects nothing and
 *              transform_indices is not looked at.
 *   M2. store     (:63)  The engine's R8 `selection_silhouette_mask` is here one bit per pixel: bit x % 64 of word x / 64 of row y of
 *              mask_bits, u64 [height][ceil(width / 64)]; the bits past `width` in a row's last word are written as zero.  When
 *              mask_attachment is not null it receives the engine's image as well, u8 [height][width], 255 for selected and 0 otherwise.
 * Stage OXC_HIGHLIGHT_COMPOSITE (highlight_dilate_horizontal.slang, highlight_composite.slang), per pixel (x, y); mask(x, y) is the bit of
 * mask_bits (bits past `width` in a row's last word are ignored):
 *   H1. dilation  (highlight_dilate_horizontal.slang:26-35, highlight_composite.slang:33-41)  rx = max(1, dilate_radius), ry = max(1,
 *              outline_width);  dilated = any mask bit in [x - rx, x + rx] x [y - ry, y + ry] cut to the image.  Cutting equals the
 *              Slang's clamped loads: a clamped tap repeats an edge pixel the window already holds, and the maximum of the rows' maxima
 *              is the maximum over the rectangle.  Stated limit, the Slang has none: rx and ry are at most 255.  The engine's
 *              `temp_horiz_dilated_mask` has no other reader and is not produced.
 *   H2. edge      (:44-45)  edge = dilated && !mask(x, y).  This is the Slang's max_mask - center_mask > 0.01 exactly: both are 0.0 or 1.0.
 *   H3. back      (:47)  Stated rule: the linear sampler at the pixel centre of an image of the same extent is the load of texel (x, y) of
 *              color_attachment.  color_format as oxc_apply_tonemap's output_format (0: R8G8B8A8 Srgb, 1: B8G8R8A8 Srgb, 2: R8G8B8A8
 *              Unorm).  The Srgb formats decode a colour byte as oxc_apply_debug_view's Albedo rule (oxc_apply_pbr step 2); format 2 and
 *              every alpha byte are f32(byte) / 255.0f.
 *   H4. outline   (:49-64)  only when edge.  is_occluded = depth(x, y) > 0.00001f (a NaN is not occluded).  final_outline =
 *              (srgb_to_linear(outline_color.rgb), outline_color.a), srgb_to_linear as written at common/color.slang:75-77: c < 0.04045f
 *              ? c / 12.92f : pow(|c + 0.055f| / 1.055f, 2.4f) -- a strict comparison, unlike the decode's -- evaluated once on the host.
 *              is_occluded and occluded_mode == 0: the back colour.  is_occluded and occluded_mode == 1: back + (final_outline - back) *
 *              0.35f per channel, alpha included.  Everything else, any other mode value included: final_outline.
 *   H5. blend     Stated rule (the vuk headers that define them are not part of the reference tree): the pass draws with
 *              vuk::BlendPreset::eAlphaBlend -- colour factors SrcAlpha / OneMinusSrcAlpha, alpha factors One / OneMinusSrcAlpha -- onto an
 *              image cleared to vuk::Black<f32>, taken as (0, 0, 0, 1).  src is the outline colour of H4 for an edge pixel and the back
 *              colour for every other.  out.rgb = src.rgb * src.a per channel: the destination term 0 * (1 - src.a) is dropped (stated; it
 *              differs only for a non-finite alpha).  out.a = src.a + (1.0f - src.a).  The store is oxc_apply_tonemap step 11 for
 *              color_format, a NaN stores 0.  A pixel that is no edge and whose alpha byte is 255 comes back with its four bytes
 *              (tests/test_highlight_model.py shows it for every byte and format), so the kernel copies such words.
 * Inputs: an input the selected stages do not read is not read, not checked and may be null.  The mask reads visbuffer_attachment,
 * transform_indices (selected_count > 0) and the frame's meshlet_instances_buffer and mesh_instances_buffer; the composite reads mask_bits,
 * depth_attachment and color_attachment.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its
 * own): struct_size; stages non-zero with no unknown bit; width and height non-zero and at most 65536; color_format 0 .. 2 and rx, ry at
 * most 255 (composite); the depth attachment one R32F level at offset 0 of width x height (composite); `frame` non-null (mask); then
 * every buffer the stages touch in the order of the context's fields, then the frame's two -- non-null (mask_attachment may be), then
 * aligned (mask_bits 8 bytes, mask_attachment 1, the others 4), then large enough (one texel per pixel; selected_count u32; height *
 * ceil(width / 64) u64; meshlet_instance_count records of 8 bytes; mesh_instances_buffer as given); then no buffer a stage writes shares
 * a byte with another buffer the call touches.  Floats are taken as given, NaN included.  One launch per stage, no scratch beyond the
 * caller's mask_bits, no allocation, no host synchronisation; capturable into a HIP graph. */
typedef struct oxc_pick_context {
  uint32_t struct_size; /* sizeof(oxc_pick_context) */
  uint32_t width, height;
  uint32_t x, y;                    /* the picking texel */
  uint32_t terrain_transform_index; /* P */
  uint32_t meshlet_instance_count;  /* P */
  oxc_buffer visbuffer_attachment;  /* in: u32[height][width] */
  oxc_buffer transform_id;          /* out: one u32 */
} oxc_pick_context;

oxc_status oxc_pick_transform(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_pick_context* context, void* hip_stream);

#define OXC_HIGHLIGHT_MASK 1u
#define OXC_HIGHLIGHT_COMPOSITE 2u
typedef struct oxc_highlight_context {
  uint32_t struct_size; /* sizeof(oxc_highlight_context) */
  uint32_t stages;      /* OXC_HIGHLIGHT_* */
  uint32_t width, height;
  uint32_t color_format;            /* H3, H5: 0: R8G8B8A8 Srgb;  1: B8G8R8A8 Srgb;  2: R8G8B8A8 Unorm */
  uint32_t terrain_transform_index; /* P */
  uint32_t meshlet_instance_count;  /* P */
  uint32_t selected_count;          /* M1 */
  float outline_color[4];           /* H4: (1.0, 0.53, 0.0, 1.0), ViewportPanel.cpp:1307 */
  int32_t dilate_radius;            /* H1: 8, the horizontal radius (ViewportPanel.cpp:1273) */
  int32_t outline_width;            /* H1: 5, the vertical radius */
  int32_t occluded_mode;            /* H4: 0 hide behind walls, 1 faded behind walls, 2 always visible (the engine's value) */
  oxc_buffer visbuffer_attachment;  /* mask in: u32[height][width] */
  oxc_buffer transform_indices;     /* mask in: u32[selected_count] */
  oxc_buffer mask_bits;             /* mask out, composite in: u64[height][ceil(width / 64)] */
  oxc_buffer mask_attachment;       /* mask out, may be null: u8[height][width] */
  oxc_image depth_attachment;       /* composite in: R32F, levels = 1 */
  oxc_buffer color_attachment;      /* composite in: u32[height][width], what oxc_apply_tonemap wrote */
  oxc_buffer dst_attachment;        /* composite out: u32[height][width], color_format */
} oxc_highlight_context;

oxc_status oxc_apply_highlight(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_highlight_context* context, void* hip_stream);

/* ---- the 2D pass: sprites and particles between oxc_apply_pbr and oxc_apply_fxaa ------------------------------------------------------------
 * oxc_draw_sprites is the 2D block of the reference's frame (RendererInstance.cpp:1080-1223, between apply_pbr :1072 and the FXAA pass :1225):
 * the passes `2d_forward_vis_pass` (passes/2d_forward_vis.slang) and `2d_forward_pass` (passes/2d_forward.slang) over one DrawBatch2D of
 * GPU::SpriteGPUData (include/Scene/SceneGPU.hpp:455-558), filled and sorted by the host at RendererInstance.cpp:1473-1532 -- here
 * oxc_pack_sprite and oxc_sort_sprites.  oxc_pick_sprite is the editor's mouse_picking_2d stage (editor/mouse_picking_2d.slang).
 * Arithmetic: the conventions of oxc_draw_visbuffer's block for everything up to the depth, and of oxc_apply_pbr's block for the colour --
 * binary32, round to nearest even, the Slang's order, no contraction, IEEE division; a comparison with a NaN operand is false.
 *
 * oxc_pack_sprite (host, plain memory) is RenderQueue2D::add (SceneGPU.hpp:532-545): material_id16_ypos16 = u16(material_id) | half(position_y)
 * << 16, flags16_distance16 = u16(render_flags) | half(distance) << 16, transform_id as given.  half() is the round-to-nearest-even binary32 ->
 * binary16 conversion with denormals kept, every NaN 0x7E00; glm::packHalf1x16 stands there in the reference.  OXC_INVALID_ARG for a null `out`.
 * oxc_sort_sprites (host, plain memory) is RenderQueue2D::sort with SpriteGPUData::operator> (SceneGPU.hpp:473-506, :547): descending by the
 * 64-bit key (distance bits << 32) | ykey, ykey = half_sort_key(ypos bits) when OXC_SPRITE_SORT_Y is set in the sprite's flags and 0 otherwise,
 * half_sort_key(b) = (b & 0x8000) ? (~b & 0xFFFF) : (b | 0x8000).  The distance is compared by its raw bits, as the reference does.  Stated
 * rule, the library's decision: the sort is stable -- sprites with equal keys keep their submission order; the reference's std::ranges::sort
 * leaves their order open.  count == 0 is valid (`sprites` may be null then); otherwise OXC_INVALID_ARG for a null `sprites`.
 *
 * oxc_draw_sprites runs the stages of `stages` over sprites [first_sprite, first_sprite + sprite_count) of sprites_buffer; with both set
 * OXC_SPRITES_VIS runs first, as in the engine.
 *   S1. fetch     (2d_forward.slang:29-59, 2d_forward_vis.slang:28-58)  flags = low 16 bits of flags16_distance16; material index = low 16 bits
 *              of material_id16_ypos16; a material index >= material_count uses the all-zero Material, as in oxc_decode_visbuffer.  Stated
 *              rule: a sprite whose transform_id >= transform_count is dropped whole (the Slang reads past the buffer).  The world matrix is
 *              transforms_world_buffer[transform_id] of `frame`, read as oxc_draw_visbuffer reads it.
 *   S2. colour    (2d_forward.slang:62-78)  sample_albedo_color without the image branch, as everywhere in this library: HasAlbedoImage is
 *              ignored, and uv, uv_size, uv_offset, ddx and ddy, which feed only the sample, are not computed.  color = the four dequantized
 *              halves of albedo_color (com::dequantize_half: a denormal half is a signed zero), linear.  The fragment is discarded when
 *              color.w <= get_alpha_cutoff(); a NaN on either side does not discard.  The test is uniform per sprite and is decided once per
 *              sprite.  The all-zero Material has 0 <= 0 and is therefore always discarded.
 *   S3. corners   (:42-55)  The six vertices are the Slang's `positions` table, (-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (0.5, 0.5), (-0.5, 0.5),
 *              (-0.5, -0.5); x is negated when OXC_SPRITE_FLIP_X is set.  world.r = ((W_r0 x + W_r1 y) + W_r2 * 0.0f) + W_r3, the `* 0` term
 *              included; clip = mul(projection_view, (world.xyz, 1)) as oxc_draw_visbuffer's vertex rule.  Two triangles, (v0, v1, v2) then
 *              (v3, v4, v5), in that order.
 *   S4. raster    The rules of oxc_draw_visbuffer, unchanged and from the same device header: the five clip planes (w >= 2^-10, |x|, |y| <= 64 w)
 *              and the fan of the clipped polygon from its corner 0, the 1/256 snap, pixel centres at (px + 0.5, py + 0.5), integer edge
 *              functions, the top-left rule, depth ((e0 z0 + e1 z1) + e2 z2) * (1 / area) in binary64 rounded once to binary32.  cullMode eNone
 *              (RendererInstance.cpp:1117, :1182): a triangle of either orientation is drawn, negative area swaps corners 1 and 2; zero area is
 *              dropped.  A fragment is kept when its depth is in (0, 1], as in the visbuffer draw.
 *   S5. order     Per pixel the fragments run in this order: sprites in buffer order from first_sprite; within a sprite triangle 0, then
 *              triangle 1; within a clipped triangle the fan order.  Each fragment does  if (d >= depth[pixel]) { depth[pixel] = d; write }
 *              (depth test eGreaterOrEqual with depth write, RendererInstance.cpp:1108-1110, :1173-1175) -- a binary32 comparison with what the attachment holds at that
 *              moment, false for a NaN.  VIS writes visbuffer_2d[pixel] = transform_id (2d_forward_vis.slang:76); COLOR blends.
 *   S6. blend     Stated rule, as H5 of oxc_apply_highlight: vuk::BlendPreset::eAlphaBlend (RendererInstance.cpp:1181) is colour SrcAlpha / OneMinusSrcAlpha and alpha One /
 *              OneMinusSrcAlpha.  dst = the stored texel decoded to binary32 (source_format 0: the exact UF11 / UF11 / UF10 decode; 1: the four
 *              halves, denormals kept).  out.c = src.c * src.a + dst.c * (1.0f - src.a), each product rounded, then the sum; source_format 1
 *              also out.a = src.a + dst.a * (1.0f - src.a); source_format 0 has no alpha and drops that result.  The result is stored by step
 *              12 of oxc_apply_pbr for the format (truncating small floats; halves round to nearest even, a NaN 0x7E00).  The store happens
 *              after every fragment: the quantisation to the attachment's format sits between two sprites on one pixel, as a ROP does it (the
 *              kernel keeps the pixel in registers as its stored word and decodes it again for the next fragment).
 *   S7. stages    With OXC_SPRITES_VIS | OXC_SPRITES_COLOR the colour stage tests against the depth the vis stage left: only fragments at the
 *              pixel's final depth blend, in order when several are equal; a translucent sprite behind the front one does not show through.
 *              OXC_SPRITES_COLOR alone is the ordered depth-tested blend.  This is the engine's behaviour (both passes share the depth
 *              attachment with eGreaterOrEqual) and it surprises people.
 * `clear` != 0 fills visbuffer_2d with ~0u first, the engine's clear (RendererInstance.cpp:644) folded in; it has a meaning only with
 * OXC_SPRITES_VIS.  sprite_count == 0 is valid: only `clear` acts.
 * Limits (else OXC_INVALID_ARG, nothing launched, nothing written; the first broken rule in this order gives the message, each has its own):
 * struct_size; stages non-zero with no unknown bit; width and height non-zero and at most 16384 (the guard band of S4 is built for that);
 * source_format 0 or 1 (OXC_SPRITES_COLOR); first_sprite + sprite_count does not wrap 32 bits and sprite_count is at most 1048576 (2^20; stated,
 * the Slang has no cap); depth_attachment is one R32F level at offset 0 of width x height; `frame` non-null; then every buffer the stages
 * touch in the order of the context's fields, then the frame's transforms_world_buffer -- non-null (materials_buffer may be when material_count
 * is 0), then aligned (4 bytes; final_attachment 8 with source_format 1), then large enough (first_sprite + sprite_count records of 12 bytes;
 * material_count records of 56; one texel per pixel; transform_count matrices of 64 bytes); then no buffer the call writes shares a byte with
 * another buffer it touches.  visbuffer_2d is touched by OXC_SPRITES_VIS only and final_attachment by OXC_SPRITES_COLOR only; an input a stage
 * does not read is not checked.  Floats are taken as given, NaN included.
 * Scratch comes from the context (576 + 136 bytes per sprite of the call, 4 bytes per 128 x 128 pixel bin and per entry of a bin's list of
 * at most 2048): the first call, or one with more sprites or bins than any before, allocates and is refused while the stream is being
 * captured -- make one un-captured call first.  After that: three launches, no allocation, no host synchronisation, capturable into a HIP
 * graph; no atomic takes part in any result, two runs over the same input are byte-identical.
 *
 * oxc_pick_sprite writes texel (x, y) of visbuffer_2d as one u32 to transform_id (mouse_picking_2d.slang:18-24: both branches store the
 * same word).  Limits as oxc_pick_transform's without the frame: struct_size; width and height non-zero and at most 65536; x < width and
 * y < height; visbuffer_2d and transform_id non-null, 4-byte aligned, large enough; transform_id shares no byte with visbuffer_2d. */
#define OXC_SPRITE_SORT_Y 1u /* RENDER_FLAGS_2D_SORT_Y */
#define OXC_SPRITE_FLIP_X 2u /* RENDER_FLAGS_2D_FLIP_X */
typedef struct oxc_sprite { /* GPU::SpriteGPUData, 12 bytes */
  uint32_t material_id16_ypos16;
  uint32_t flags16_distance16;
  uint32_t transform_id;
} oxc_sprite;

oxc_status oxc_pack_sprite(uint32_t render_flags, float position_y, uint32_t transform_id, uint32_t material_id, float distance, oxc_sprite* out);
oxc_status oxc_sort_sprites(oxc_sprite* sprites, uint64_t count);

#define OXC_SPRITES_VIS 1u
#define OXC_SPRITES_COLOR 2u
typedef struct oxc_sprite_context {
  uint32_t struct_size; /* sizeof(oxc_sprite_context) */
  uint32_t stages;      /* OXC_SPRITES_* */
  uint32_t width, height;
  uint32_t clear;         /* != 0: visbuffer_2d is filled with ~0u first (OXC_SPRITES_VIS) */
  uint32_t source_format; /* S6: 0: B10G11R11 UfloatPack32;  1: R16G16B16A16 Sfloat, as oxc_apply_fxaa */
  uint32_t first_sprite, sprite_count; /* one DrawBatch2D */
  uint32_t material_count;             /* S1 */
  uint32_t transform_count;            /* S1 */
  float projection_view[16];           /* S3: column-major */
  oxc_buffer sprites_buffer;           /* in: oxc_sprite[first_sprite + sprite_count] */
  oxc_buffer materials_buffer;         /* in: GPU::Material[material_count], 56 bytes each */
  oxc_image depth_attachment;          /* in/out: R32F, levels = 1 */
  oxc_buffer visbuffer_2d;             /* vis out: u32[height][width] */
  oxc_buffer final_attachment;         /* colour in/out: u32[height][width] or u16[height][width][4], what oxc_apply_pbr wrote */
} oxc_sprite_context;

oxc_status oxc_draw_sprites(oxc_ctx* ctx, const oxc_prepared_frame* frame, const oxc_sprite_context* context, void* hip_stream);

typedef struct oxc_sprite_pick_context {
  uint32_t struct_size; /* sizeof(oxc_sprite_pick_context) */
  uint32_t width, height;
  uint32_t x, y;           /* the picking texel */
  oxc_buffer visbuffer_2d; /* in: u32[height][width] */
  oxc_buffer transform_id; /* out: one u32 */
} oxc_sprite_pick_context;

oxc_status oxc_pick_sprite(oxc_ctx* ctx, const oxc_sprite_pick_context* context, void* hip_stream);

/* ---- multi-GPU exchange: one process per GPU, RCCL over xGMI ---------------------------
 * The meshlet-instance array shards by contiguous range and every rank culls its shard on its own; the only
 * exchanges of the path are (1) the per-rank counters {emitted meshlets, early, late, index count} to every rank
 * (16 bytes per rank) so that each can place its compacted buffers in a merged list, and (2) the HiZ pyramid from
 * the rank that owns the depth buffer.  These entry points are those two collectives on the caller's stream,
 * through RCCL (loaded with dlopen, so the single-GPU path does not need the library).
 *   rank 0: oxc_comm_unique_id(id) -> the launcher hands the 128 bytes to the other ranks (any side channel)
 *   all:    oxc_comm_init(ctx, id, rank, world)                                                          */
#define OXC_COMM_UNIQUE_ID_BYTES 128
oxc_status oxc_comm_unique_id(oxc_ctx* ctx, void* id128_host_out);
oxc_status oxc_comm_init(oxc_ctx* ctx, const void* id128_host, uint32_t rank, uint32_t world);
oxc_status oxc_comm_destroy(oxc_ctx* ctx);
/* Packs the counters of `context`'s last oxc_cull_geometry call -- {meshlets emitted (cull_triangles_cmd.x), early, late
 * (visibility_buffer), index_count (draw_geometry_cmd)} -- into counts4_dptr (device, u32[4]) on the stream: the input of
 * oxc_exchange_counts, without a host round trip.  Usable on one GPU as well. */
oxc_status oxc_pack_counters(oxc_ctx* ctx, const oxc_cull_geometry_context* context, void* counts4_dptr, void* hip_stream);
/* The same for the `count` (<= 16) contexts of one oxc_cull_geometry_batch call in ONE launch: counts4_dptr[i][4] = element i's
 * {emitted, visibility.total (the length of the view's MeshletInstance list), late, index_count} -- configs[4] sharded over ranks all-gathers
 * these per view. */
oxc_status oxc_pack_counters_batch(oxc_ctx* ctx, uint32_t count, const oxc_cull_geometry_context* contexts, void* counts4_dptr, void* hip_stream);
/* all-gather of 4 u32 per rank: counts4_dptr (this rank's {emitted, early, late, index_count}) -> all_counts_dptr[world][4] */
oxc_status oxc_exchange_counts(oxc_ctx* ctx, const void* counts4_dptr, void* all_counts_dptr, void* hip_stream);
/* broadcast of every level of `hiz` from rank `root` (in place) */
oxc_status oxc_broadcast_hiz(oxc_ctx* ctx, const oxc_image* hiz, uint64_t total_bytes, uint32_t root, void* hip_stream);
/* The "top mips" form of the same exchange: only levels >= first_level travel (bytes [level_offset[first_level], total_bytes) of the
 * linear chain: 5.6 MB instead of 89.5 MB for a 4096^2 pyramid with first_level = 2).  A rank must hold EVERY level it may sample
 * (clamping the mip would change results), so this form is for ranks that own a copy of the depth image and build levels
 * < first_level themselves: oxc_generate_hiz with hiz_attachment.levels = first_level.  The pyramid is a pure function of the depth
 * image, so both forms give every rank the same bytes. */
oxc_status oxc_broadcast_hiz_levels(oxc_ctx* ctx, const oxc_image* hiz, uint32_t first_level, uint64_t total_bytes, uint32_t root, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OXCULL_H */
