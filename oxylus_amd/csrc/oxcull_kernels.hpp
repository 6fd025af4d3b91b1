// oxcull_kernels.hpp -- kernel argument blocks and launcher prototypes shared by the kernel TU
// (oxcull_kernels.hip) and the C-ABI host TUs (oxcull_abi_*.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "oxcull.h"
#include "oxcull_types.hpp"

namespace oxc {

struct PrepareArgs {
  const GpuMesh* meshes;
  const float* transforms;
  GpuMeshInstance* mesh_instances;
  InstCache* cache;
  uint32_t* mesh_counts;
  uint32_t* slot;          // this call's counter slot
  uint32_t* vis;           // {total, early, late}
  uint32_t* meshlets_cmd;  // {x,1,1}
  uint32_t* supers_meshlets;
  uint32_t* supers_tris;
  uint32_t n_supers_meshlets, n_supers_tris;
  uint32_t* tickets;  // kTicketCounters work counters (stride kSuperStride) zeroed here for the test kernels that take work dynamically; may be null
  // share_pass_tests, early call: the late call of the frame will reuse this call's instance rows, so everything else its prepare
  // kernel would do is done here -- a second set of accumulators and its counter slot -- and the late call launches none.  Null: not armed.
  uint32_t* slot_late;
  uint32_t* supers_meshlets_late;
  uint32_t* supers_tris_late;
  uint32_t* tickets_late;
  uint32_t mesh_instance_count;
  uint32_t cull_flags;
  uint32_t do_cull_meshes;
  uint32_t init_vis;    // write vis/meshlets_cmd initial values
  uint32_t seed_total;  // initial vis.total (0 for the reference flow)
  oxc_cull_camera cam;
  // multi-view (use_hpb): blockIdx.y = 1 + v computes rows view_cache[v * M + mi] with
  // clipmaps[v].projection_view_mat in place of the camera matrix
  const oxc_virtual_clipmap* clipmaps;
  InstCache* view_cache;
};

struct HpbTestArgs {
  const InstCache* cache;
  const InstCache* view_cache;
  const GpuMeshletInstance* meshlet_instances;
  const uint32_t* vis;
  uint64_t* bits;
  uint32_t* chunk_counts;
  uint32_t* supers;
  uint32_t* tickets;  // work counters (zeroed by prepare)
  const oxc_virtual_clipmap* clipmaps;
  const uint32_t* dirty;
  uint32_t clipmap_count;
  uint32_t mesh_instance_count;
  uint32_t n_cap;  // frame.max_meshlet_instance_count: the device-side list length is clamped to what the buffers hold
  const uint8_t* hpb_data;
  uint32_t hpb_w, hpb_h, hpb_layers, hpb_levels;
  uint32_t hpb_level_off[13];
  float light_dir[3];  // camera.position carries -light_dir
};

struct MeshletTestArgs {
  uint32_t n_host;  // != 0: the list length is known on the host (seeded lists); skips the dependent load of vis[0]
  uint32_t n_cap;   // frame.max_meshlet_instance_count: vis[0] is clamped to what the scratch and the output lists hold
  uint32_t mask_bits;  // bits the visibility mask buffer holds; mask indices beyond it read as "not visible" and are never written
  const InstCache* cache;
  const GpuMeshletInstance* meshlet_instances;
  const uint32_t* vis;
  uint32_t* mask;
  uint64_t* bits;
  uint32_t* chunk_counts;
  uint32_t* supers;
  uint32_t* tickets;  // != null: waves take their 64*G-meshlet steps from these counters instead of a fixed stride (zeroed by prepare)
  // Two-pass sharing (oxc_cull_geometry_context::share_pass_tests): the early HiZ call leaves, per 64-meshlet group, the ballot of
  // "passed the frustum and the normal-cone test" (the tests that depend on the camera only) and, per wave step, where its run of mask
  // bits starts; the late call of the same frame reads them instead of testing again.  share: 0 = off, 1 = write them (early call),
  // 2 = read them (late call).
  uint32_t share;
  // unordered_output (include/oxcull.h), plain kernel only: the test kernel appends its survivors itself -- slot allocation by atomic_add as
  // the reference does (cull_meshlets.slang:55-70), aggregated per block through the ballots -- and no emit kernel runs.
  // out = visible_meshlet_instances_indices, count_a = cull_triangles_cmd.x.  Null `out`: the ordered two-launch form.
  uint32_t* out;
  uint32_t* count_a;
  uint32_t* dbg_occlusion;     // measurement aid (null: off): 256 counters, stride kSuperStride words, the counting instantiations add the candidates that reach test_occlusion
  uint64_t* camera_test_bits;  // [ceil(N / 64)]
  uint2* step_info;        // [steps]: {first mask bit of the step, 1 if the step's 64 * G meshlets are one run of mask bits}
  const float* hiz_data;
  uint32_t hiz_level_off[13];  // float offsets of each mip
  uint32_t hiz_w, hiz_h, hiz_levels;
  uint32_t hiz_lds_first;     // first level staged in LDS (== hiz_levels: none)
  uint32_t hiz_lds_off[13];   // float offset of each staged level inside the LDS tile
  float near_clip;
  float cam_pos[3];
};

struct MeshletEmitArgs {
  uint32_t n_host;
  uint32_t n_cap;
  uint32_t count_meshlets;  // meshlets per published count (64 * groups-per-wave of the test kernel that ran)
  const uint64_t* bits;
  const uint32_t* chunk_counts;
  const uint32_t* supers;
  uint32_t* vis;
  uint32_t* tri_cmd;
  uint32_t* out;  // visible_meshlet_instances_indices
};

struct TriTestArgs {
  const InstCache* cache;
  const GpuMeshletInstance* meshlet_instances;
  const uint32_t* visible;
  const uint32_t* vis;
  const uint32_t* tri_cmd;
  uint64_t* tri_masks;
  uint32_t* chunk_counts;
  uint32_t* supers;
  float resolution[2];  // cull_camera.resolution: read by the small-triangle variants only
  // unordered_output: the fused kernel (test + expansion of a kFusedTriSpan-meshlet span in one launch; slots by atomic_add on index_count, as
  // cull_triangles.slang:71-88 does per workgroup) writes the packed indices and the draw command itself
  uint32_t* draw_cmd;
  uint32_t* out;  // reordered_indices
  // round 5, fused kernel: the chunks of the last, partial round of the grid are drawn from these counters (tris_fused_body; zeroed by the
  // prepare kernel: the ordered form's triangle super-chunk accumulators, which the fused form does not use)
  uint32_t* ticket;
  uint32_t ticket_count;  // counters behind `ticket` (stride kSuperStride words), >= 1
};

struct TriEmitArgs {
  const uint64_t* tri_masks;
  const uint32_t* visible;
  const uint32_t* vis;
  const uint32_t* tri_cmd;
  const uint32_t* chunk_counts;
  const uint32_t* supers;
  uint32_t* draw_cmd;
  uint32_t* out;  // reordered_indices
};

struct ScanArgs {
  const uint32_t* counts;
  uint32_t* offsets;
  uint32_t n;
  uint32_t cap;  // frame.max_meshlet_instance_count: the expansion stops there
  uint32_t* vis;
  uint32_t* meshlets_cmd;
};

struct ExpandArgs {
  const uint32_t* counts;
  const uint32_t* offsets;
  uint32_t n;
  uint32_t cap;
  GpuMeshletInstance* out;
};

// Argument blocks of one oxc_cull_geometry_batch call (plain pipeline, <= kMaxBatch independent
// frames).  Passed by value to the batched prepare kernel, which copies it to the context's device
// buffer; every later kernel of the call reads its element through blockIdx.y from there.
constexpr uint32_t kMaxBatch = 16;      // elements per batched call
constexpr uint32_t kBatchPerPrepare = 16;  // element cores (BatchCore) per kernarg segment of k_prepare_batch
struct BatchElem {
  PrepareArgs prep;
  ScanArgs scan;
  ExpandArgs expand;
  MeshletTestArgs test;
  MeshletEmitArgs emit;
  TriTestArgs ttest;
  TriEmitArgs temit;
};
// What the host hands over per element: every pointer and scalar of BatchElem exactly once (the seven stage
// blocks repeat them 2-5 times).  k_prepare_batch rebuilds the stage blocks from it on the device
// (expand_batch_core), so a kernarg segment carries kBatchPerPrepare = 8 elements instead of 5.
struct BatchCore {
  // caller buffers
  const GpuMesh* meshes;
  const float* transforms;
  GpuMeshInstance* mesh_instances;
  GpuMeshletInstance* meshlet_instances;
  uint32_t* visible_out;    // visible_meshlet_instances_indices
  uint32_t* reordered_out;  // reordered_indices
  // the element's scratch lane
  InstCache* cache;
  InstCache* view_cache;
  uint32_t* mesh_counts;
  uint32_t* mesh_offsets;
  uint64_t* bits;
  uint32_t* m_chunk_counts;
  uint32_t* m_supers;
  uint64_t* tri_masks;
  uint32_t* t_chunk_counts;
  uint32_t* t_supers;
  // counters
  uint32_t* slot;  // tri_cmd / draw_cmd live at slot + SLOT_TRI_CMD / SLOT_DRAW_CMD
  uint32_t* vis;
  uint32_t* meshlets_cmd;
  uint32_t n_supers_meshlets, n_supers_tris;
  uint32_t mesh_instance_count;
  uint32_t cull_flags;
  uint32_t do_cull_meshes;
  uint32_t init_vis;
  uint32_t n_host;
  uint32_t n_cap;
  uint32_t count_meshlets;  // meshlets per published count of the test kernel (64 * groups per wave)
  oxc_cull_camera cam;
};
// What one k_prepare_batch launch receives by value: up to kBatchPerPrepare elements, which it expands to
// dev[first .. first + count) and prepares (blockIdx.y = element).
struct BatchBlob {
  BatchCore core[kBatchPerPrepare];
  uint32_t count;
  uint32_t first;
};
static_assert(sizeof(BatchBlob) <= 8000, "must fit the kernarg segment");

// The stage blocks of one element from its core (the only place that knows which block needs which field).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void prepare_args_of(const BatchCore& c, PrepareArgs& pa) {
  pa.meshes = c.meshes;
  pa.transforms = c.transforms;
  pa.mesh_instances = c.mesh_instances;
  pa.cache = c.cache;
  pa.mesh_counts = c.mesh_counts;
  pa.slot = c.slot;
  pa.vis = c.vis;
  pa.meshlets_cmd = c.meshlets_cmd;
  pa.supers_meshlets = c.m_supers;
  pa.supers_tris = c.t_supers;
  pa.tickets = nullptr;  // batched elements run the plain meshlet test (fixed stride)
  pa.slot_late = nullptr;
  pa.supers_meshlets_late = pa.supers_tris_late = pa.tickets_late = nullptr;
  pa.n_supers_meshlets = c.n_supers_meshlets;
  pa.n_supers_tris = c.n_supers_tris;
  pa.mesh_instance_count = c.mesh_instance_count;
  pa.cull_flags = c.cull_flags;
  pa.do_cull_meshes = c.do_cull_meshes;
  pa.init_vis = c.init_vis;
  pa.seed_total = 0;
  pa.cam = c.cam;
  pa.clipmaps = nullptr;
  pa.view_cache = c.view_cache;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void expand_batch_core(const BatchCore& c, BatchElem& e) {
  uint32_t* tri_cmd = c.slot + SLOT_TRI_CMD;
  uint32_t* draw_cmd = c.slot + SLOT_DRAW_CMD;
  prepare_args_of(c, e.prep);
  e.scan = ScanArgs{c.mesh_counts, c.mesh_offsets, c.mesh_instance_count, c.n_cap, c.vis, c.meshlets_cmd};
  e.expand = ExpandArgs{c.mesh_counts, c.mesh_offsets, c.mesh_instance_count, c.n_cap, c.meshlet_instances};
  MeshletTestArgs& ta = e.test;
  ta.n_host = c.n_host;
  ta.n_cap = c.n_cap;
  ta.mask_bits = 0;
  ta.cache = c.cache;
  ta.meshlet_instances = c.meshlet_instances;
  ta.vis = c.vis;
  ta.mask = nullptr;
  ta.bits = c.bits;
  ta.chunk_counts = c.m_chunk_counts;
  ta.supers = c.m_supers;
  ta.out = ta.count_a = nullptr;  // batched elements keep the ordered form
  ta.dbg_occlusion = nullptr;
  ta.hiz_data = nullptr;
  ta.hiz_w = ta.hiz_h = ta.hiz_levels = ta.hiz_lds_first = 0;
  ta.near_clip = c.cam.near_clip;
  ta.cam_pos[0] = c.cam.position[0];
  ta.cam_pos[1] = c.cam.position[1];
  ta.cam_pos[2] = c.cam.position[2];
  MeshletEmitArgs& ea = e.emit;
  ea.n_host = c.n_host;
  ea.n_cap = c.n_cap;
  ea.count_meshlets = c.count_meshlets;
  ea.bits = c.bits;
  ea.chunk_counts = c.m_chunk_counts;
  ea.supers = c.m_supers;
  ea.vis = c.vis;
  ea.tri_cmd = tri_cmd;
  ea.out = c.visible_out;
  TriTestArgs& tt = e.ttest;
  tt.cache = c.cache;
  tt.meshlet_instances = c.meshlet_instances;
  tt.visible = c.visible_out;
  tt.vis = c.vis;
  tt.tri_cmd = tri_cmd;
  tt.tri_masks = c.tri_masks;
  tt.chunk_counts = c.t_chunk_counts;
  tt.supers = c.t_supers;
  tt.resolution[0] = c.cam.resolution[0];
  tt.resolution[1] = c.cam.resolution[1];
  tt.draw_cmd = tt.out = nullptr;
  tt.ticket = nullptr;
  tt.ticket_count = 0;
  TriEmitArgs& te = e.temit;
  te.tri_masks = c.tri_masks;
  te.visible = c.visible_out;
  te.vis = c.vis;
  te.tri_cmd = tri_cmd;
  te.chunk_counts = c.t_chunk_counts;
  te.supers = c.t_supers;
  te.draw_cmd = draw_cmd;
  te.out = c.reordered_out;
}

// ---- multi-view meshlet stage: oxc_cull_geometry_batch over several VIEWS of one scene (cull_meshes + cull_meshlets per view) ----
// One pass over the scene's meshlets instead of one per view: the views that kept a mesh instance at the same LOD form a group,
// a wave loads a 256-meshlet chunk of the group's bounds records once and tests it against every view of the group
// (cull_meshlets_hpb.slang:59-79 is the reference's own one-thread-many-views shape).  Per view the output is what the per-view
// kernels write: the view's own ascending list of indices into the view's own MeshletInstance list.
struct MvView {
  const InstCache* rows;         // this view's instance rows (prepare_body with this view's camera)
  const uint32_t* mesh_counts;   // [M] meshlets of the instance in this view's list (0: culled by this view's cull_meshes)
  const uint32_t* mesh_offsets;  // [M] first record of the instance in this view's list
  uint32_t* vchunks;             // [M] 256-meshlet chunks of the instance in this view ...
  uint32_t* vchunk0;             // [M] ... and their exclusive prefix: the view's own chunk numbering
  uint64_t* bits;                // [chunks][4] survivor ballots per view chunk
  uint32_t* counts;              // [chunks]
  uint32_t* idbase;              // [chunks] list index of the chunk's first meshlet
  uint32_t* supers;              // per 64 chunks (stride kSuperStride)
  uint32_t* scan_total;          // [2] number of chunks of this view
  uint32_t* out;                 // visible_meshlet_instances_indices of this view
  uint32_t* runs;                // [M][2] optional: {first, count} of the instance in this view's (possibly implicit) MeshletInstance list
  uint32_t* tri_cmd;
  uint32_t n_cap;                // the view's list capacity
  uint32_t n_supers;
  float cam_pos[3];
  uint32_t _pad;
};
struct MvGroup {  // the views of one mesh instance that read the same bounds array with the same transform and the same count
  uint64_t bounds;
  uint32_t count;
  uint32_t view_mask;
};
struct MvBlob {
  MvView v[kMaxBatch];
};
struct MvArgs {
  uint32_t views, M;
  uint32_t same_pos;  // every view has the same camera position: the normal cone is evaluated once per meshlet, not once per view
  MvView* dev;        // device copy of the table (written by k_mv_group)
  MvGroup* groups;    // [M][views]
  uint32_t* grp_chunks;  // [M] chunks of all groups of the instance
  uint32_t* inst_step0;  // [M] exclusive prefix
  uint32_t* step_total;  // [2]
  uint2* steps;          // [total] {mesh instance, group | chunk << 8}
  uint32_t* tickets;
};
void launch_mv_setup(const MvArgs& a, const MvBlob& blob, uint32_t grid, hipStream_t s);  // groups, chunk numbering, step list
void launch_mv_test(const MvArgs& a, uint32_t num_cus, hipStream_t s);
void launch_mv_emit(const MvArgs& a, uint32_t max_chunks_per_view, uint32_t max_grid, hipStream_t s);

struct HizArgs {
  const float* depth;
  float* hiz;
  uint32_t dw, dh;
  uint32_t w, h, levels;
  uint32_t level_off[13];  // floats
};

void launch_prepare(const PrepareArgs& a, uint32_t grid, uint32_t views, hipStream_t s);
void launch_hpb_test(const HpbTestArgs& a, uint32_t grid, hipStream_t s);
void launch_scan_mesh_counts(const uint32_t* counts, uint32_t* offsets, uint32_t n, uint32_t cap, uint32_t* vis, uint32_t* cmd, hipStream_t s);
void launch_expand(const uint32_t* counts, const uint32_t* offsets, uint32_t n, uint32_t cap, void* out, uint32_t grid, hipStream_t s);
// grid_limit != 0: at most that many blocks (async_triangles: the HiZ variants leave wave slots to the triangle stage running beside them)
// a.out != null: the unordered (appending) instantiation of the same kernel; no emit launch follows
void launch_meshlets_test(const MeshletTestArgs& a, bool hiz, bool occl, bool late, uint32_t grid, uint32_t num_cus, uint32_t grid_limit, hipStream_t s);
void launch_meshlets_emit(const MeshletEmitArgs& a, bool hiz, bool late, uint32_t grid, hipStream_t s);
void launch_tris_test(const TriTestArgs& a, bool late, bool wide, bool small_triangle_cull, bool cached_loads, uint32_t grid, hipStream_t s);  // cached_loads: shared (instanced) geometry -- plain loads instead of `nt`
void launch_tris_emit(const TriEmitArgs& a, bool late, uint32_t wide, uint32_t grid, hipStream_t s);  // wide: oxc_cull_geometry_context::wide_triangle_index (0, 1, 2 = pairs)
// unordered_output: test + expansion in one launch (a.draw_cmd / a.out set); grid in kFusedTriSpan-meshlet spans
void launch_tris_fused(const TriTestArgs& a, bool late, uint32_t wide, bool small_triangle_cull, bool cached_loads, uint32_t grid, uint32_t resident_cus, hipStream_t s);
void launch_hiz(const HizArgs& a, uint32_t num_cus, hipStream_t s);
// batched (grid.y = batch element); `dev` is the device copy written by launch_prepare_batch
void launch_prepare_batch(const BatchBlob& blob, BatchElem* dev, uint32_t grid, hipStream_t s);
void launch_scan_batch(const BatchElem* dev, uint32_t count, hipStream_t s);
void launch_expand_batch(const BatchElem* dev, uint32_t count, uint32_t grid, hipStream_t s);
void launch_meshlets_test_batch(const BatchElem* dev, uint32_t count, uint32_t grid, hipStream_t s);
void launch_meshlets_emit_batch(const BatchElem* dev, uint32_t count, uint32_t grid, hipStream_t s);
void launch_tris_test_batch(const BatchElem* dev, uint32_t count, uint32_t grid, hipStream_t s);
void launch_tris_emit_batch(const BatchElem* dev, uint32_t count, uint32_t grid, hipStream_t s);
void launch_seed_slot(uint32_t* slot, uint32_t total, hipStream_t s);
void launch_pack_counters(const uint32_t* vis, const uint32_t* tri_cmd, const uint32_t* draw_cmd, uint32_t* out4, hipStream_t s);
struct PackBlob {  // one element per context of a batched call (null pointers read as 0)
  const uint32_t* vis[kMaxBatch];
  const uint32_t* tri_cmd[kMaxBatch];
  const uint32_t* draw_cmd[kMaxBatch];
  uint32_t count;
};
void launch_pack_counters_batch(const PackBlob& blob, uint32_t* out4, hipStream_t s);
void launch_stream_read(const void* p, uint64_t bytes, uint32_t* sink, uint32_t grid, hipStream_t s);
void launch_debug_decode_bounds(const void* bounds, uint32_t n, float* out10, hipStream_t s);
struct DebugProjectArgs {
  float mvp[16];
  float near_clip;
  uint32_t n;
  const float* boxes6;
  float* out7;
};
void launch_debug_project_aabb(const DebugProjectArgs& a, hipStream_t s);
// oxcull_raster.hip: consumer of the indirect draw
struct TriSetup;
// What vs_main needs of a mesh instance, resolved once per draw by k_draw_rows (mesh_instance -> mesh -> lods[lod] is three dependent
// loads per vertex otherwise): the LOD's arrays and rows 0..2 of the world matrix.
struct DrawRow {
  uint64_t meshlets, micro, vidx, positions;
  float w[12];
};
struct DrawArgs {
  float pv[16];
  DrawRow* rows;
  uint32_t mesh_instance_count;
  const GpuMesh* meshes;
  const float* transforms;
  const GpuMeshInstance* mesh_instances;
  const GpuMeshletInstance* meshlet_instances;
  const uint32_t* indices;    // reordered_indices
  const uint32_t* draw_cmd;   // VkDrawIndexedIndirectCommand: [0] = indexCount
  unsigned long long* visdepth;
  uint32_t width, height;
  uint32_t wide;
  // Big triangles (pixel box beyond the small path) are queued in kBigSegs segments of the big list, each with its own counter
  // (stride kBigSegStride words): a single counter retires ~13 ns per wave-level atomic on this part, which serialised the setup kernel.
  uint32_t big_seg_capacity;  // triangles per segment
  TriSetup* big_list;
  uint32_t* big_seg_counts;
  uint32_t clip_capacity;  // triangles that cross a clip plane: ids queued for k_draw_clipped
  uint32_t* clip_list;
  uint32_t* clip_count;
  uint32_t tile_capacity;  // 64 x 64 pixel tiles of the big triangles' boxes: {big list index, tile} pairs, one wave each in k_draw_big
  uint2* tile_list;
  uint32_t* tile_count;
};
void launch_draw_visbuffer(const DrawArgs& a, bool clear, float* depth_out, uint32_t* vis_out, uint32_t max_grid, hipStream_t s);
// its launches around the draw's own kernels, which oxc_draw_terrain takes as well: the clears (image with `clear`, scratch header always), the
// big list with its tiles, the optional resolve.  They read visdepth, width, height and the big / tile / clip fields of `a`.
void launch_draw_clear(const DrawArgs& a, bool clear, uint32_t max_grid, hipStream_t s);
void launch_draw_big(const DrawArgs& a, uint32_t max_grid, hipStream_t s, uint32_t* fragments = nullptr);  // fragments: the counting instantiations add theirs to it
void launch_resolve_visbuffer(const DrawArgs& a, float* depth_out, uint32_t* vis_out, uint32_t max_grid, hipStream_t s);
constexpr uint32_t kTriSetupBytes = 40;
constexpr uint32_t kBigSegs = 256, kBigSegStride = 16;
constexpr uint32_t kRasterHeaderBytes = 256 + kBigSegs * kBigSegStride * 4;  // clip / tile counters, then the segment counters
// oxcull_terrain.hip: terrain patch cull
struct TerrainArgs {
  float pv[16];
  float near_clip;
  uint32_t cull_flags;
  float world_min[2], world_size[2];
  uint32_t pcx, pcy;
  float base_height, height_scale;
  const float2* patch_minmax;
  const float* hiz_data;
  uint32_t hiz_level_off[13];
  uint32_t hiz_w, hiz_h, hiz_levels;
  uint32_t* mask;
  uint32_t* visible;
  uint32_t* draw_cmd;
  // scratch of the two-kernel form (more than 1024 patches): one emit ballot per wave, one count per 1024-patch block
  uint64_t* emit_bits;
  uint32_t* block_counts;
};
void launch_cull_terrain(const TerrainArgs& a, hipStream_t s);
// oxcull_hpb.hip: hierarchical page buffer producer
void launch_generate_hpb(const uint32_t* page_table, uint8_t* data, uint32_t w, uint32_t h, uint32_t layers, uint32_t levels, const uint64_t* level_offset,
                         hipStream_t s);
// oxcull_vsm.hip: VSM page update (oxc_update_virtual_shadowmap)
struct VsmArgs {
  uint32_t* page_table;  // [layers][n][n]
  const float* clipmaps; // GPU::VirtualClipmap[layers], 19 words each
  const float* depth;
  uint32_t depth_w, depth_h, depth_vec4;  // depth_vec4: rows may be read with 16-byte loads (width % 4 == 0, 16-byte aligned)
  uint32_t n, layers, page_size, phys_side, phys_count;  // phys_side = P = physical_page_table_size / page_size
  uint32_t sun_moved, invalidate;
  // pass 3 (invalidate); the counts bound every index read on the device
  const uint32_t* dirty_ids;
  uint32_t dirty_count, mesh_instance_count, mesh_count, transform_count, transform_previous_count;
  const GpuMeshInstance* mesh_instances;
  const GpuMesh* meshes;
  const float* transforms;
  const float* transforms_previous;
  // outputs
  uint32_t* dirty_flags;
  uint32_t* dirty_coords;  // u32x2 per dirty page
  uint32_t* clear_cmd;
  uint32_t* counters;
  float* physical;  // optional: physical_size x physical_size R32F
  uint32_t physical_size;
  // context scratch
  uint8_t* mark;  // [layers][n][n]: 1 = marked visible by this call's pixel pass
  uint32_t* free_list;
  // pixel pass constants, computed once per call on the host in binary32 / binary64 (include/oxcull.h)
  float inv_pv[16];
  float off_x, off_y;  // (1.0 / resolution) * 0.5
  float texel_len;
  uint32_t lvl_always;  // k < lvl_always: (double)k - bias < 0, always counted
  float lvl_thr[16];    // k >= lvl_always: counted when r > lvl_thr[k] (binary32 round-down of exp2(k - bias): the same decision as the binary64 compare)
};
// reset + invalidate, mark, resolve (free / allocate / dirty list), then the optional HPB (hpb != nullptr) and clear (a.physical != nullptr)
void launch_vsm_update(const VsmArgs& a, uint32_t num_cus, uint8_t* hpb, uint32_t hpb_levels, const uint64_t* hpb_level_offset, hipStream_t s);
// oxcull_vsm_draw.hip: the VSM shadow draw (oxc_draw_physical_pages)
struct VsmBig {  // a (triangle, clipmap) pair whose pixel box is beyond the in-wave path: snapped corners, oriented with positive area
  int32_t x[3], y[3];
  float z[3];
  uint32_t layer;
};
struct VsmDrawArgs {
  DrawRow* rows;  // [mesh_instance_count], written by the call
  uint32_t mesh_instance_count;
  const GpuMesh* meshes;
  const float* transforms;
  const GpuMeshInstance* mesh_instances;
  const GpuMeshletInstance* meshlet_instances;
  const uint32_t* indices;   // reordered_indices
  const uint32_t* draw_cmd;  // VkDrawIndexedIndirectCommand
  uint32_t wide;             // wide_triangle_index
  uint32_t max_triangles;    // triangles reordered_indices_buffer holds
  const uint32_t* page_table;  // [layers][n][n]
  const float* clipmaps;       // GPU::VirtualClipmap[layers], 19 words each
  const uint32_t* dirty_flags;
  uint32_t n, layers, page_size, phys_side, V;  // phys_side = P = physical_page_table_size / page_size, V = n * page_size
  int32_t ps_shift;                             // log2(page_size) when a power of two, else -1
  uint32_t words_per_layer;                     // n * n / 32
  float* physical;  // physical_size x physical_size R32F
  uint32_t physical_size;
  uint32_t* out_cmds;  // optional (all three or none)
  uint32_t* out_count;
  uint32_t* out_clipmaps;
  // context scratch
  uint32_t* header;   // active count + list, queue counters, statistics
  uint32_t* bitmap;   // [layers][words_per_layer]: drawable virtual pages of the active clipmaps
  uint32_t* pagemap;  // [layers][n][n]: physical page coords (x | y << 16) of a drawable virtual page, else all ones
  VsmBig* big_list;
  uint32_t big_capacity;
  uint2* clip_list;  // {triangle, clipmap}
  uint32_t clip_capacity;
  uint2* tile_list;  // {big list index, virtual page vy * n + vx}
  uint32_t tile_capacity;
};
constexpr uint32_t kVsmDrawHeaderBytes = 1024;
void launch_vsm_draw(const VsmDrawArgs& a, bool stats, uint32_t max_grid, hipStream_t s);
// oxcull_vsm_resolve.hip: the VSM shadow resolve (oxc_resolve_shadowmap)
struct VsmResolveArgs {
  const float* depth;        // [h][w]
  const uint32_t* normal;    // u16x4 [h][w] as two words per pixel: {r | g << 16, b | a << 16}
  float* out;                // [h][w]
  uint32_t w, h;
  const float* clipmaps;       // GPU::VirtualClipmap[layers], 19 words each
  const uint32_t* page_table;  // [layers][n][n]
  const float* physical;       // physical_size x physical_size R32F
  uint32_t n, layers, page_size, phys_side, phys_count, physical_size;  // phys_side = P = physical_page_table_size / page_size
  float fn, fV;                // float(n), float(n * page_size)
  uint32_t* stats;             // nullptr, or u32[8] the counting instantiation adds to (oxc_debug_vsm_resolve_stats)
  // per-call constants, computed once on the host in binary32 / binary64 by the rules of include/oxcull.h
  float inv_pv[16];
  float off_x, off_y;  // (1.0 / resolution) * 0.5
  float texel_len;
  uint32_t lvl_always;  // as VsmArgs
  float lvl_thr[16];
  float light[3], tangent[3], bitangent[3];  // L and perpendicular_basis(L)
  float z_length, inv_z_length;
  float ham[40][2];  // hammersley2d(i, 16), i < 16, then hammersley2d(i, 24), i < 24
};
void launch_vsm_resolve(const VsmResolveArgs& a, hipStream_t s);
// oxcull_contact_shadows.hip: the contact shadow ray march (oxc_contact_shadows)
struct ContactShadowsArgs {
  const float* depth;  // [h][w]
  float* out;          // [h][w]
  uint32_t w, h;
  float fw, fh;        // float(w), float(h)
  uint32_t steps;
  uint32_t* stats;     // nullptr, or u32[12] the counting instantiation adds to (oxc_debug_contact_shadows_stats)
  // per-call constants, computed once on the host in binary32 by the rules of include/oxcull.h
  float inv_pv[16], view[16], proj[16];
  float ray[3];           // normalize(sun_dir) * shadow_length
  float depth_thickness;  // thickness * (1.0 / near_clip)
  float one_plus_bias;    // 1.0f + 0.000002f
  float edge_span;        // 0.3f - 1.0f, smoothstep's edge1 - edge0
};
void launch_contact_shadows(const ContactShadowsArgs& a, hipStream_t s);
// oxcull_ambient_occlusion.hip: VBGTAO prefilter, main and denoise (oxc_generate_ambient_occlusion)
struct AmbientOcclusionArgs {
  const float* depth;       // [h][w] device depth
  const uint32_t* normal;   // [h][w] u16x4 as two words
  const uint16_t* hilbert;  // [64][64]
  float* pre;               // prefiltered_depth: five levels
  uint32_t* edges;          // depth_differences [h][w]
  uint16_t* noisy;          // noisy_occlusion [h][w], binary16
  uint16_t* out;            // ambient_occlusion_attachment [h][w], binary16
  uint32_t* stats;          // nullptr, or u32[15] the counting instantiation of the main kernel adds to (oxc_debug_ambient_occlusion_stats)
  uint64_t lvl_off[5];      // first float of each level
  uint32_t lvl_w[5], lvl_h[5];
  uint32_t w, h;
  uint32_t slice_count, samples, noise_add;  // noise_add = 288 * (noise_index % 64)
  // per-call constants, computed once on the host in binary32 by the rules of include/oxcull.h
  float lin_mul, lin_add;  // projection[3][2], projection[2][2] (glm indexing)
  float pf_mul, pf_add;    // the prefilter's falloff pair
  float view3[9];          // view's upper 3 x 3, row by row
  float p00, p11, res_x, res_y;
  float far_thr;           // far_clip * 0.999f
  float thickness, slice_count_f, samples_f;
  float falloff_mul, falloff_add;
  float radius_x, radius_y;  // (0.5f * effect_radius') * |p00|, * |p11|
  float final_power;
};
void launch_ambient_occlusion(const AmbientOcclusionArgs& a, hipStream_t s);
// oxcull_visbuffer_decode.hip: the G-buffer images from the visibility buffer (oxc_decode_visbuffer)
struct VisbufferDecodeArgs {
  const uint32_t* vis;         // [h][w]
  const uint32_t* depth_bits;  // [h][w]: the R32F depth's bit patterns (only "is it 0" is read)
  uint32_t* albedo;            // [h][w] R8G8B8A8 sRGB
  uint2* normal;               // [h][w] R16G16B16A16 Sfloat as two words: {r | g << 16, b | a << 16}
  uint32_t* emissive;          // [h][w] B10G11R11 UfloatPack32
  uint32_t* mro;               // [h][w] R8G8B8A8 Unorm
  uint32_t w, h;
  float fw, fh;                // float(w), float(h)
  uint32_t clear;
  uint32_t meshlet_instance_count, material_count;
  const GpuMeshletInstance* meshlet_instances;
  const GpuMeshInstance* mesh_instances;
  const GpuMesh* meshes;
  const float* transforms;     // 16-byte aligned
  const uint32_t* materials;   // GPU::Material[material_count], 14 words each
  uint32_t* stats;             // nullptr, or u32[4] the counting instantiation adds to (oxc_debug_visbuffer_decode_stats)
  float pv[16];
};
void launch_visbuffer_decode(const VisbufferDecodeArgs& a, hipStream_t s);
// oxcull_visbuffer_decode_textured.hip: the same with the five material images sampled (oxc_decode_visbuffer_textured)
struct MaterialImage {  // oxc_material_image
  uint64_t dptr;
  uint32_t width, height, levels, format;
  uint64_t level_offset[15];
};
static_assert(sizeof(MaterialImage) == 144, "layout");
struct VisbufferDecodeTexturedArgs {
  VisbufferDecodeArgs g;        // stats: nullptr, or u32[13] (oxc_debug_visbuffer_decode_textured_stats)
  float camera_position[3];
  uint32_t image_count, sampler_count;
  const MaterialImage* images;  // [image_count]
  const uint32_t* samplers;     // [sampler_count][4]: {filter, address, mip_filter, _pad}, 4-byte aligned
};
void launch_visbuffer_decode_textured(const VisbufferDecodeTexturedArgs& a, hipStream_t s);
// oxcull_pbr_apply.hip: the lit HDR image from the G-buffer and the shadow terms (oxc_apply_pbr)
struct PbrApplyArgs {
  const float* depth;       // [h][w]
  const uint32_t* albedo;   // [h][w] R8G8B8A8 sRGB
  const uint2* normal;      // [h][w] u16x4 as two words: {r | g << 16, b | a << 16}
  const uint32_t* emissive; // [h][w] B10G11R11 UfloatPack32
  const uint32_t* mro;      // [h][w] R8G8B8A8 Unorm
  const uint16_t* ao;       // [h][w] binary16
  const float* resolved;    // [h][w], read with HasDirectionalLight
  const float* contact;     // [h][w], read with HasContactShadows
  const void* lights;       // GPU::Light[light_count], 64 bytes each
  void* out;                // [h][w] u32 (B10G11R11), or uint2 (R16G16B16A16 Sfloat) with TransparentBackground
  uint32_t* stats;          // nullptr, or u32[9] the counting instantiation adds to (oxc_debug_pbr_apply_stats)
  uint32_t w, h;
  float fw, fh;             // float(w), float(h)
  uint32_t flags;           // GPU::SceneFlags
  uint32_t light_count;
  float inv_pv[16];
  float camera[3], sun[3], sun_intensity;
  // selected once on the host (no arithmetic): HasSky ? sky_ambient_color : base_ambient_color;  sky_has_texture ? (1, 1, 1) : sky_solid_color.rgb
  float env[3], sky_color[3];
};
void launch_pbr_apply(const PbrApplyArgs& a, hipStream_t s);
// the atmosphere branch (oxc_apply_pbr_atmosphere): `g` as above without stats, env and sky_color; the four sky images and what of the rule
// depends on the call alone, evaluated once on the host by pbr_atmosphere_constants() in the binary32 operations the header states
struct PbrAtmosphereArgs {
  PbrApplyArgs g;
  const uint2* transmittance;  // [th][tw] u16x4
  const uint2* sky_view;       // [vh][vw]
  const uint2* aerial;         // [ad][ah][aw]
  const uint2* cube;           // [6][cube_size][cube_size]
  uint32_t tw, th, vw, vh, aw, ah, ad, cube_size;
  float planet_radius, atmos_radius;
  float h_atmos, eye_altitude, beta, zenith_horizon_angle;  // AtmosphereConstants, from camera_position.y
  float min_altitude;                                       // planet_radius + 0.001f
  float sun_cos_theta, horizon_darkening;                   // dot(L, up); smoothstep(-0.1f, 0.3f, sun_cos_theta)
  float min_cos;                                            // draw_sun: the cos rule at (1.0f * PI) / 180.0f
  float aerial_depth;                                       // f32(aerial_perspective_lut_size.z)
  float inv_per_slice_depth, inv_aerial_depth;              // 1.0f / (lut.x / lut.z), 1.0f / lut.z
  float near_depth_fade_out;                                // 1.0f / 0.001f
  float aerial_start_km, aerial_exposure;
};
void pbr_atmosphere_constants(const oxc_atmosphere& atm, PbrAtmosphereArgs& a);  // fills everything below `cube` but the AtmosphereConstants; reads a.g.sun
void launch_pbr_apply_atmosphere(const PbrAtmosphereArgs& a, hipStream_t s);
// oxcull_eye_adaptation.hip: the luminance histogram of the lit HDR image and the exposure it gives (oxc_apply_eye_adaptation)
struct EyeAdaptationArgs {
  const void* src;       // `pixels` texels in one run: u32 (B10G11R11, format 0) or u16x4 (R16G16B16A16 Sfloat, format 1)
  uint32_t* histogram;   // u32[256], zeroed by the first launch
  float* exposure;       // {adapted_luminance, exposure}, read and written by the averaging kernel
  uint64_t pixels;       // width * height
  uint64_t vectors;      // whole 16-byte vectors behind the head
  uint32_t head;         // texels before the first 16-byte boundary
  uint32_t format;
  float min_exposure, exposure_range;  // max_exposure - min_exposure, one binary32 subtraction on the host
  float pixel_count;     // f32(width * height)
  float time_coeff, ev100_bias;
};
void launch_eye_adaptation(const EyeAdaptationArgs& a, uint32_t grid, hipStream_t s);
// oxcull_bloom.hip: the bloom prefilter and the two mip pyramids (oxc_apply_bloom)
struct BloomArgs {
  const void* src;        // W x H texels: u32 (B10G11R11, format 0) or u16x4 (R16G16B16A16 Sfloat, format 1)
  const float* exposure;  // the exposure buffer's {adapted_luminance, exposure}; nullptr: the exposure is 1.0
  void* down[13];         // D: level k is max(1, w2 >> k) x max(1, h2 >> k) texels of the source's format
  void* up[13];           // U
  uint32_t w, h;          // the source's extent
  uint32_t w2, h2;        // w / 2, h / 2: the extent of level 0
  uint32_t levels;        // L
  uint32_t tail;          // T in 1 .. L: the tail kernel runs downsample levels T .. L - 1 and upsample levels L - 1 .. T; L: no tail kernel
  uint32_t format;
  float threshold, soft_threshold, clamp_value, radius;
};
uint32_t bloom_default_tail(uint32_t w2, uint32_t h2, uint32_t levels);
uint32_t bloom_lowest_tail(uint32_t w2, uint32_t h2, uint32_t levels);  // the lowest T OXC_TUNE_BLOOM_TAIL_LEVEL can force
void launch_bloom(const BloomArgs& a, hipStream_t s);
// oxcull_tonemap.hip: exposure, bloom composite, tone curve, lens effects and the 8-bit store (oxc_apply_tonemap)
// What of the tone curves and of FfxLensGetRGMag does not depend on the pixel (step 5 of the header block): evaluated once per call on the
// host by tonemap_constants(), binary32 in the Slang's order.
struct TonemapConstants {
  float agx_in[9], agx_out[9];  // sRGB_to_adjusted and its inverse, row-major
  float agx_s, agx_span, agx_neg_c, agx_peak;  // color_DualSection: S = peak * linear, peak - S, -(peak / (peak - S)), peak
  float gt_sdr, gt_target, gt_target_ucs;      // sdrCorrectionFactor_, framebufferLuminanceTarget_, framebufferLuminanceTargetUcs_
  float gt_mid, gt_toe, gt_ka, gt_kb, gt_kc;   // midPoint_, toeStrength_, kA_, kB_, kC_
  float gt_lin_peak, gt_mid_span;              // linearSection_ * peakIntensity_, midPoint_ - 0.0
  float gt_blend, gt_one_minus_blend, gt_fade_start, gt_fade_end, gt_fade_span;
  float pq_m2, pq_inv_m2, pq_inv_m1;           // 78.84375 * exponentScaleFactor, 1.0 / m2, 1.0 / m1
  float red_mag, green_mag;                    // FfxLensGetRGMag(chromatic_aberration_amount)
};
struct TonemapArgs {
  const void* src;        // w x h texels: u32 (B10G11R11, format 0) or u16x4 (R16G16B16A16 Sfloat, format 1)
  const void* bloom;      // U level 0, bw x bh texels of the source's format; read with HasBloom
  const float* exposure;  // {adapted_luminance, exposure}; read with HasEyeAdaptation
  uint32_t* dst;          // [h][w]
  uint32_t w, h, bw, bh;
  uint32_t flags, format, output_format, tonemap_type;
  float exposure_setting, vignette_amount, grain_scale, grain_amount, bloom_intensity;
  uint32_t grain_seed;
  uint32_t grain_divisor;  // the saturating truncation of grain_scale / 8.0f, 0 taken as 1
  TonemapConstants k;
};
void tonemap_constants(float chromatic_aberration_amount, TonemapConstants& k);
void launch_tonemap(const TonemapArgs& a, hipStream_t s);
// oxcull_fxaa.hip: edge anti-aliasing of the lit HDR image (oxc_apply_fxaa)
struct FxaaArgs {
  const void* src;  // w x h texels: u32 (B10G11R11, format 0) or u16x4 (R16G16B16A16 Sfloat, format 1)
  void* dst;        // the same extent and format
  uint32_t w, h, format;
  uint32_t* stats;  // nullptr, or u32[4] the counting instantiation adds to (oxc_debug_fxaa_stats)
};
void launch_fxaa(const FxaaArgs& a, hipStream_t s);
// oxcull_atmosphere.hip: the four sky LUTs (oxc_generate_sky_luts, oxc_draw_atmosphere)
// What does not depend on the texel (the header block's "host constants"): evaluated once per call by atmosphere_constants() in binary64 from
// the binary32 arguments, each rounded to binary32 once.
struct AtmosphereConstants {
  float h_atmos;                       // sqrt(max(0, atmos_radius^2 - planet_radius^2))
  float g_hg, g_d, alpha, w_d;         // the four exp constants of henyey_greenstein_draine_phase
  float eye_altitude;                  // Atmosphere::get_eye_pos(camera.position).y, also length(eye_pos)
  float beta, zenith_horizon_angle;    // acos(horizon / eye_altitude), pi - beta
};
struct SkyLutInputs {
  oxc_atmosphere atm;
  AtmosphereConstants k;
  const uint2* transmittance;  // read by the multiscattering, sky-view and aerial passes
  const uint2* multiscatter;   // bound as the reference binds it; read only by an instantiation with eval_multiscattering
};
struct SkyLutArgs {
  SkyLutInputs in;
  const float* hemisphere;  // 64 x float3
  uint2* transmittance;     // out, == in.transmittance
  uint2* multiscatter;      // out
};
struct AtmosphereArgs {
  SkyLutInputs in;
  float sun_dir[3], sun_intensity;
  float camera_position[3];
  float inv_projection_view[16];
  uint2* sky_view;  // out
  uint2* aerial;    // out, [depth][height][width]
  uint32_t slice_blocks;  // blocks per aerial slice, filled by launch_atmosphere
};
void atmosphere_constants(const oxc_atmosphere& atm, const float* camera_y, AtmosphereConstants& k);  // camera_y nullptr: the camera terms stay 0
void launch_sky_luts(const SkyLutArgs& a, hipStream_t s);
void launch_atmosphere(AtmosphereArgs a, hipStream_t s);
// the sky cubemap (oxc_generate_sky_ibl); in.multiscatter is not bound
struct SkyIblArgs {
  SkyLutInputs in;
  float sun_dir[3], sun_intensity, sun_ambient_strength;
  uint32_t frame_index, cube_size, texels;  // texels = 6 * cube_size^2
  const uint2* sky_view;
  uint2* cube;  // in and out, [6][cube_size][cube_size]
};
void launch_sky_ibl(const SkyIblArgs& a, hipStream_t s);
// oxcull_terrain_maps.hip: the terrain maps (oxc_generate_terrain_maps); the folded values are the header block's "the host may evaluate"
struct TerrainMapsArgs {
  oxc_terrain_generate g;
  oxc_terrain_derive d;
  uint32_t res[2], patches[2];
  uint32_t threads_texels[2], threads_patches[2];  // roundup(dispatch, 16 / 8), capped at roundup(resolution / patch_count): multiples of 16 / 8
  float fres[2];                // f32(resolution)
  float strength0, freq0;       // E.strength * E.scale; 1.0f / (E.scale * E.cell_scale)
  float one_minus_norm;         // 1.0f - E.normalization
  float amp06;                  // G.height_amplitude * 0.6f
  float den[2];                 // 8.0f * D.texel_world_size
  float mm_scale[2];            // f32(resolution) / f32(patch_count)
  const uint32_t* region;       // nullptr: both origins zero
  uint16_t* heightmap;
  uint16_t* ridgemap;
  uint32_t* normalmap;
  uint32_t* splatmap;
  const float* height_edit;
  const uint32_t* splat_edit;
  float2* patch_minmax;
};
void terrain_maps_constants(TerrainMapsArgs& a);  // fills the folded values from g, d, res and patches
void launch_terrain_generate(const TerrainMapsArgs& a, hipStream_t s);
void launch_terrain_derive(const TerrainMapsArgs& a, hipStream_t s);
void launch_terrain_minmax(const TerrainMapsArgs& a, hipStream_t s);
// oxcull_terrain_brush.hip: the terrain brush (oxc_apply_terrain_brush); the kernels evaluate the direction and the span themselves
struct TerrainBrushArgs {
  oxc_terrain_brush_params p;
  uint32_t groups;  // of 16 x 16 threads a side: (2 * u32(ceil(radius_texels)) + 1 + 15) / 16, at most 513
  const uint16_t* heightmap;
  float* height_edit;
  uint32_t* splat_edit;
  uint32_t* hit;     // {f32 world_position[3], u32 valid}: written by trace, read by apply
  uint32_t* region;  // {texel_origin.xy, patch_origin.xy}
};
void launch_terrain_brush_trace(const TerrainBrushArgs& a, hipStream_t s);
void launch_terrain_brush_apply(const TerrainBrushArgs& a, hipStream_t s);
// oxcull_terrain_decode.hip: the G-buffer of the terrain pixels (oxc_decode_terrain)
struct TerrainDecodeArgs {
  uint32_t w, h;
  float fw, fh;
  float ipv[16];         // Camera::inv_projection_view, column-major
  oxc_terrain_data t;    // GPU::TerrainData; the decode reads world_min, inv_world_size, layer_material_indices, brush_radius
  uint32_t map_w, map_h, material_count;
  const uint32_t* vis;
  const float* depth;
  const uint32_t* normalmap;  // one word per texel: two binary16, x in the low half
  const uint32_t* splatmap;   // R8G8B8A8 Unorm, R in the low byte
  const uint32_t* materials;  // 14 words a record
  const uint32_t* hit;        // {f32 world_position[3], u32 valid}; not read unless brush_radius > 0
  uint32_t* albedo;
  uint2* normal;
  uint32_t* emissive;
  uint32_t* mro;
};
void launch_terrain_decode(const TerrainDecodeArgs& a, hipStream_t s);
// oxcull_terrain_draw.hip: the tessellated terrain patches into the depth|vis image (oxc_draw_terrain)
constexpr uint32_t kTerrainStatsWord = 8;  // the call's eight counters are words 8 .. 15 of the raster scratch header, zeroed with it
struct TerrainDrawArgs {
  DrawArgs r;  // pv, visdepth, width, height and the big / tile lists of the shared raster scratch; the mesh fields stay null
  float camera_position[3], near_clip, projection_scale;
  oxc_terrain_data t;
  uint32_t map_w, map_h;
  const uint16_t* heightmap;
  const uint32_t* visible;    // visible_patches
  uint64_t visible_capacity;  // its entries
  const uint32_t* draw_cmd;   // VkDrawIndirectCommand: [1] = instanceCount, [3] = firstInstance
  uint32_t* stats;            // u32[8]
};
void launch_draw_terrain(const TerrainDrawArgs& a, bool clear, bool count_fragments, float* depth_out, uint32_t* vis_out, uint32_t max_grid, hipStream_t s);
// oxcull_debug_view.hip: the debug views (oxc_apply_debug_view)
struct DebugViewArgs {  // the main views, OXC_DEBUG_VIEW_TRIANGLES .. OXC_DEBUG_VIEW_GEOMETRIC_NORMAL
  uint32_t w, h, clear, meshlet_instance_count;
  float heatmap_scale;
  const uint32_t* vis;
  const float* depth;
  // what the selected view reads; the others are null
  const uint32_t* overdraw;
  const uint32_t* albedo;
  const uint2* normal;  // {r | g << 16, b | a << 16}
  const uint32_t* emissive;
  const uint32_t* mro;
  const uint16_t* ao;
  const GpuMeshletInstance* meshlet_instances;
  const GpuMeshInstance* mesh_instances;
  const GpuMesh* meshes;
  uint2* out;  // u16x4 [h][w]
};
void launch_debug_view(uint32_t view, const DebugViewArgs& a, hipStream_t s);
struct DebugViewVsmArgs {  // OXC_DEBUG_VIEW_RMVSM
  const float* depth;
  uint2* out;
  uint32_t w, h;
  const float* clipmaps;       // GPU::VirtualClipmap[layers], 19 words each
  const uint32_t* page_table;  // [layers][n][n]
  uint32_t n, layers, page_size;
  float fn, fphys;             // float(n), float(physical_page_table_size)
  float hue_divisor;           // f32(clipmap_count + 1)
  // as VsmResolveArgs: clipmap_selection_constants fills them
  float inv_pv[16];
  float off_x, off_y;
  float texel_len;
  uint32_t lvl_always;
  float lvl_thr[16];
};
void launch_debug_view_vsm(const DebugViewVsmArgs& a, hipStream_t s);
// oxcull_highlight.hip: the editor's selection path (oxc_pick_transform, oxc_apply_highlight)
struct HighlightRecords {  // what resolves a visbuffer texel to a transform index
  const uint32_t* vis;     // u32 [h][w]
  const GpuMeshletInstance* meshlet_instances;
  const GpuMeshInstance* mesh_instances;
  uint32_t w, h, meshlet_instance_count, terrain_transform_index;
};
struct PickArgs {
  HighlightRecords r;
  uint32_t x, y;
  uint32_t* out;
};
void launch_pick_transform(const PickArgs& a, hipStream_t s);
struct HighlightMaskArgs {
  HighlightRecords r;
  const uint32_t* selected;  // transform_indices[selected_count]
  uint32_t selected_count;
  uint64_t* mask_bits;       // u64 [h][ceil(w / 64)]
  uint8_t* mask_attachment;  // u8 [h][w] or null
};
void launch_highlight_mask(const HighlightMaskArgs& a, hipStream_t s);
struct HighlightCompositeArgs {
  const uint64_t* mask_bits;
  const float* depth;
  const uint32_t* color;
  uint32_t* dst;
  uint32_t w, h, format;
  uint32_t rx, ry;      // H1: max(1, dilate_radius), max(1, outline_width)
  int32_t occluded_mode;
  float outline[4];     // H4: final_outline, evaluated by highlight_outline_linear
};
void highlight_outline_linear(const float* outline_color, float* final_outline);
void launch_highlight_composite(const HighlightCompositeArgs& a, hipStream_t s);
// the pow rule on the host (oxcull_tonemap.hip keeps the host's copy of the log2 rule)
float pow_rule_host(float v, float p);
// oxcull_sprites.hip: the 2D pass (oxc_draw_sprites, oxc_pick_sprite)
constexpr uint32_t kSpriteBin = 128;           // side of a coarse bin in pixels; one block of k_sprites_bin per bin
constexpr uint32_t kSpriteTile = 16;           // side of a tile in pixels; one block of k_sprites_pixels per tile, one pixel per lane
constexpr uint32_t kSpriteChunk = 256;         // sprites a block tests per step of its ordered compaction (bin and tile kernels alike)
constexpr uint32_t kSpriteBinCapacity = 2048;  // entries of a bin's list; a bin that meets more makes its tiles walk the sprite records themselves
constexpr uint32_t kSpriteMaxTris = 12;        // fan triangles of a sprite that crosses clip planes: 6 per source triangle
constexpr uint32_t kSpriteMaxCount = 1u << 20; // sprites of one call (stated limit)
constexpr int32_t kSpriteNarrowSpread = 28672; // corner spread (1/256 px) below which every edge value of a tile the sprite touches fits edge_fn32
struct SpriteTri {  // one set-up triangle, oriented with positive area (48 bytes)
  int32_t x[3], y[3];
  float z[3];
  uint32_t inv_area_lo, inv_area_hi;  // binary64 1 / area
  uint32_t bias;                      // bit k: edge k is not inclusive
};
struct SpriteRecord {   // what a pixel needs of a sprite (128 bytes)
  float ca[3];          // S6: src.c * src.a
  float a, one_minus_a;
  uint32_t transform_id;
  uint32_t shape;       // triangle count | clipped << 8 (the triangles are in the side array) | narrow << 9
  uint32_t pad;
  SpriteTri tri[2];     // the usual sprite: two triangles inside every plane
};
struct SpriteArgs {
  const uint32_t* sprites;    // oxc_sprite records from first_sprite on
  const uint32_t* materials;  // GPU::Material[material_count], 14 words each
  const float* transforms;
  uint32_t sprite_count, material_count, transform_count;
  float pv[16];
  uint32_t w, h, stages, clear;
  uint32_t bins_x, bins_y, list_stride;  // list_stride = min(sprite_count, kSpriteBinCapacity)
  SpriteRecord* records;                 // [sprite_count]
  uint2* boxes;                          // [sprite_count] {px0 | py0 << 16, px1 | py1 << 16}; empty: {~0u, 0}
  SpriteTri* clipped;                    // [sprite_count][kSpriteMaxTris], written for sprites that cross a plane only
  uint32_t* bin_counts;                  // [bins]: the sprites whose box meets the bin (above list_stride: the list is cut short)
  uint32_t* bin_lists;                   // [bins][list_stride], ascending
  float* depth;
  uint32_t* vis;
  void* color;
};
void launch_draw_sprites(const SpriteArgs& a, uint32_t format, hipStream_t s);
void launch_pick_sprite(const uint32_t* vis, uint32_t w, uint32_t x, uint32_t y, uint32_t* out, hipStream_t s);
// oxcull_bounds.hip: meshlet bounds producer
void launch_build_meshlet_bounds(const float* pos, uint32_t vertex_count, const void* meshlets, uint32_t meshlet_count, const uint32_t* vidx,
                                 const uint8_t* micro, void* out_bounds, float* out_mesh6, void* out_qpos, float* meshlet_minmax, float* normals,
                                 uint32_t* normal_counts, float* fold_scratch, uint32_t chunk, uint32_t max_grid, uint32_t grid_cap, hipStream_t s);

void launch_quantize_vertex_streams(const float* pos, const float* nrm, const float* uv, uint32_t vertex_count, void* out_qpos, void* out_qnrm,
                                    void* out_quv, uint32_t max_grid, hipStream_t s);
}  // namespace oxc
