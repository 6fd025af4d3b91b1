/* oxcull_debug.h -- test, harness and measurement hooks of liboxcull.so.
 *
 * NOT part of the drop-in boundary: include/oxcull.h is what an engine binds (INTEGRATION.md sections 1-2, oxylus_amd/host/RendererInstance.hpp
 * includes only that).  The entry points below exist for this repo's tests (known-answer sweeps of the device's decode and projection
 * routines, read-backs, the overflow paths of the rasteriser), for bench.py (per-kernel HIP-event timing, the streaming-read ceiling,
 * SURVEY 8d's occlusion-candidate count) and for tools/kbench.py (grid caps that the A/B measurements move).  They are exported by the
 * same library; tests/test_abi.py checks both headers against the export table. */
#ifndef OXCULL_DEBUG_H
#define OXCULL_DEBUG_H
#include "oxcull.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Streaming-read probe: sums `bytes` of device memory with 16 B/lane loads (the measured HBM
 * ceiling SURVEY 8d asks to report next to the 8 TB/s spec figure). */
oxc_status oxc_stream_read_probe(oxc_ctx* ctx, const void* dptr, uint64_t bytes, void* hip_stream);

/* ---- per-kernel timing (bench / profiling; off by default) ----
 * Between oxc_profile_begin and oxc_profile_end every kernel the context launches is bracketed
 * by a pair of hipEvents on the caller's stream.  oxc_profile_end synchronises and returns, per
 * kernel, the launch count and the summed event-to-event time, plus the measured cost of an
 * empty event pair (`empty_pair_ms`, to be subtracted per launch). */
enum {
  OXC_K_PREPARE = 0,
  OXC_K_MESHES_SCAN = 1,
  OXC_K_MESHES_EXPAND = 2,
  OXC_K_MESHLETS_TEST = 3,  /* plain / early-pass variants */
  OXC_K_MESHLETS_EMIT = 4,
  OXC_K_TRIANGLES_TEST = 5,
  OXC_K_TRIANGLES_EMIT = 6,
  OXC_K_HIZ = 7,
  OXC_K_MESHLETS_TEST_LATE = 8, /* the LatePass instantiations, timed apart: their candidate sets differ */
  OXC_K_MESHLETS_EMIT_LATE = 9,
  OXC_K_TRIANGLES_TEST_LATE = 10,
  OXC_K_TRIANGLES_EMIT_LATE = 11,
  OXC_K_DRAW_VISBUFFER = 12, /* every launch of one oxc_draw_visbuffer call (clear, setup, clipped, big, resolve) */
  OXC_K_MESHLET_BOUNDS = 13, /* oxc_build_meshlet_bounds */
  OXC_K_MULTIVIEW_SETUP = 14, /* batched views of one scene: view groups per mesh instance, chunk numbering, step list (three small launches) */
  OXC_K_VSM_UPDATE = 15, /* every launch of one oxc_update_virtual_shadowmap call (reset + invalidate, mark, resolve, HPB, clear) */
  OXC_K_COUNT = 16
};
typedef struct oxc_kernel_times {
  double total_ms[16];
  uint32_t launches[16];
  double empty_pair_ms;
} oxc_kernel_times;
oxc_status oxc_profile_begin(oxc_ctx* ctx);
oxc_status oxc_profile_end(oxc_ctx* ctx, oxc_kernel_times* out);

/* Test hook: decode n GPU::MeshletBounds records with the device's dequantize_half / s8/127
 * routines into 10 floats each {center.xyz, extent.xyz, cone_axis.xyz, cone_cutoff}
 * (scene.slang:401-435) -- lets the known-answer tests sweep all 65536 halfs and 256 s8s. */
oxc_status oxc_debug_decode_bounds(oxc_ctx* ctx, const void* bounds_dptr, uint32_t n, float* out10_dptr,
                                   void* hip_stream);

/* Test hook: project_aabb (cull.slang:12-47) of n boxes {center.xyz, extent.xyz} with one matrix: out7 = {min.u, min.v,
 * min.z, max.u, max.v, max.z, returned ? 1 : 0} per box -- lets the tests compare the device's division fast path with IEEE
 * division bit for bit. */
oxc_status oxc_debug_project_aabb(oxc_ctx* ctx, const float* mvp16_host, float near_clip, const void* boxes6_dptr, uint32_t n, float* out7_dptr,
                                  void* hip_stream);

/* Harness helper: copy n u32 from device memory (e.g. a callee-owned indirect command) to the host; synchronises the stream. */
oxc_status oxc_debug_read_u32(oxc_ctx* ctx, const void* dptr, uint32_t n, uint32_t* host_out, void* hip_stream);
/* Test hook: what share_pass_tests did in the context's last oxc_cull_geometry call -- 0: the call tested on its own, 1: early call that
 * also published its results, 2: late call that reused them, 3: late call that reused them and launched no prepare kernel (the early
 * call had done that work too: it was in order on one stream and directly in front of it). */
uint32_t oxc_debug_shared_tests_mode(const oxc_ctx* ctx);
/* Test hook: which loads the triangle kernels of the context's last oxc_cull_geometry call used for vertex ids / micro indices / positions -- 0: the call
 * ran no triangle stage, 1: `nt` (geometry read once), 2: plain (geometry shared between instances: >= 4 mesh instances per Mesh record, or OXC_TUNE_TRI_LOADS). */
uint32_t oxc_debug_tri_loads_mode(const oxc_ctx* ctx);

/* Harness hook: sizing / scheduling knobs of a context that the measurements and the tests move (the library itself reads no environment
 * variable).  OXC_TUNE_ASYNC_*: resident blocks per CU the persistent kernels of the meshlet / triangle stage take while async_triangles
 * lets the two stages share the machine (0 = no limit, the default).  OXC_TUNE_RASTER_BIG_CAPACITY: entries of oxc_draw_visbuffer's
 * big-triangle / clip queues (default 2^22); only before the context's first draw, which allocates them -- the tests shrink it to reach
 * the overflow paths with a small scene. */
enum { OXC_TUNE_ASYNC_MTEST_BLOCKS_PER_CU = 0, OXC_TUNE_ASYNC_TRI_BLOCKS_PER_CU = 1, OXC_TUNE_RASTER_BIG_CAPACITY = 2,
       OXC_TUNE_TRI_BLOCKS_PER_CU = 3 /* grid cap of the triangle kernels in blocks per CU (default 8 = one resident round) */,
       OXC_TUNE_TRI_LOADS = 7 /* triangle kernels' loads of vertex ids / micro indices / positions: 0 (default) = by the scene -- plain loads when the geometry is shared (>= 4 mesh instances per Mesh record), `nt` when it is unique; 1 = always `nt`; 2 = always plain.  Same outputs either way */,
       OXC_TUNE_MV_EXPAND_ASYNC = 5 /* multi-view batch: blocks per CU of the MeshletInstance expansion on the context's own low-priority stream beside the meshlet stage (default 4); 0: in order on the caller's stream */,
       OXC_TUNE_VSM_DRAW_STATS = 8 /* 1: oxc_draw_physical_pages runs counting kernels (oxc_debug_vsm_draw_stats); 0 (default): off */,
       OXC_TUNE_VSM_DRAW_CAPACITY = 9 /* entries of oxc_draw_physical_pages' big-pair / clip queues (default: every (triangle, clipmap)
                                         pair of the frame's index buffer, 4096..2^24, growing with the frame; the tile queue holds 2x
                                         as many); fixed, only before the context's first shadow draw -- the tests shrink it to reach
                                         the overflow paths */,
       OXC_TUNE_VSM_RESOLVE_STATS = 10 /* 1: oxc_resolve_shadowmap runs its counting instantiation (oxc_debug_vsm_resolve_stats); 0 (default): off */,
       OXC_TUNE_CONTACT_SHADOWS_STATS = 11 /* 1: oxc_contact_shadows runs its counting instantiation (oxc_debug_contact_shadows_stats); 0 (default): off */,
       OXC_TUNE_AMBIENT_OCCLUSION_STATS = 12 /* 1: oxc_generate_ambient_occlusion runs the counting instantiation of its main kernel (oxc_debug_ambient_occlusion_stats); 0 (default): off */,
       OXC_TUNE_VISBUFFER_DECODE_STATS = 13 /* 1: oxc_decode_visbuffer runs its counting instantiation (oxc_debug_visbuffer_decode_stats); 0 (default): off */,
       OXC_TUNE_PBR_APPLY_STATS = 14 /* 1: oxc_apply_pbr runs its counting instantiation (oxc_debug_pbr_apply_stats); 0 (default): off */,
       OXC_TUNE_EYE_ADAPTATION_GRID = 15 /* cap of oxc_apply_eye_adaptation's histogram kernel in blocks; 0 (default): uncapped (four blocks per CU).  With it a small image makes every block run its stride loop several times.  Same outputs either way */,
       OXC_TUNE_RASTER_GRID = 18 /* cap, in blocks, of every launch of oxc_draw_visbuffer; 0 (default): uncapped (eight blocks per CU; 256 for the clip queue's kernel).  It takes effect at the next draw.  With it a small triangle list makes every wave run its stride loop several times.  Same outputs either way */,
       OXC_TUNE_VSM_DRAW_GRID = 19 /* cap, in blocks, of every launch of oxc_draw_physical_pages (the prologue's x extent, the rows kernel and the clip queue's kernel included); 0 (default): uncapped (eight blocks per CU; 256 for the clip queue's kernel).  It takes effect at the next draw.  With it a small frame makes every wave run its stride loop several times.  Same outputs either way */,
       OXC_TUNE_BOUNDS_GRID = 20 /* cap, in blocks, of every grid-stride launch of oxc_build_meshlet_bounds and oxc_quantize_vertex_streams (the quantisers, the gather kernel and the mesh fold's partial kernel, whose block count the final fold then reads; the cone kernel runs a thread per meshlet and the final fold one block, so neither has a grid to cap); 0 (default): uncapped (eight blocks per CU for the quantisers, sixteen for the gather kernel, 256 partial blocks).  It takes effect at the next call.  With it a small mesh makes every wave and every fold thread run its stride loop several times.  Same outputs either way */,
       OXC_TUNE_BOUNDS_CHUNK = 21 /* meshlets per gather / cone launch pair of oxc_build_meshlet_bounds; 0 (default): 2^18.  Only the loop's step: the scratch keeps the layout and size of the default, so a value above 2^18 (or above the rows the scratch holds) is clamped.  It takes effect at the next call.  With it a small mesh is processed in several chunks with a ragged last one.  Same outputs either way */,
       OXC_TUNE_TERRAIN_DRAW_GRID = 22 /* cap, in blocks, of every launch of oxc_draw_terrain; 0 (default): uncapped (eight blocks per CU).  It takes effect at the next draw.  With it a block takes several patches through its stride loop.  Same outputs either way */,
       OXC_TUNE_TERRAIN_DRAW_STATS = 23 /* 1: oxc_draw_terrain runs counting instantiations of its kernel and of the big-list kernels (the fragment counter of oxc_debug_terrain_draw_stats); 0 (default): off.  Same image */,
       OXC_TUNE_VISBUFFER_DECODE_TEXTURED_STATS = 24 /* 1: oxc_decode_visbuffer_textured runs its counting instantiation (oxc_debug_visbuffer_decode_textured_stats); 0 (default): off.  Same images */,
       OXC_TUNE_FXAA_STATS = 17/* 1: oxc_apply_fxaa runs its counting instantiation (oxc_debug_fxaa_stats); 0 (default): off */,
       OXC_TUNE_BLOOM_TAIL_LEVEL = 16 /* the level T from which oxc_apply_bloom's one-block tail kernel takes over (downsample levels T .. L - 1, upsample levels back to T); 0 (default): chosen by the library; a value >= L: no tail kernel, one launch per level.  A forced T is raised to the first level whose source level has at most 16 384 texels (64 per thread of the one block), so the knob cannot turn a large image into one long single-block kernel.  Same outputs either way */ };
oxc_status oxc_debug_set_tuning(oxc_ctx* ctx, uint32_t knob, uint32_t value);

/* Measurement aid: counters_dptr != NULL -- the HiZ calls (use_hiz + OXC_CULL_TEST_OCCLUSION) that follow on this context run counting
 * instantiations of their meshlet test, which ADD the number of candidates that reach test_occlusion (cull_meshlets_hiz.slang:53-65:
 * SURVEY 8d's f, four pyramid taps = 16 B each) to 256 u32 counters 256 bytes apart (u32[256 * 64], caller-zeroed; their sum is the
 * count).  Same outputs, slower kernels: not for timed runs.  NULL switches it off again. */
oxc_status oxc_debug_count_occlusion_candidates(oxc_ctx* ctx, void* counters_dptr);

/* Test hook: what the last oxc_draw_visbuffer on this context did with its triangles; synchronises the stream.
 * out4 = {triangles queued for the big path (pixel box beyond 8 x 8), triangles that crossed a clip plane, 64 x 64 tiles handed to
 * the tile list, big-list segments that overflowed (their excess triangles were walked by the setup lane: slow, correct)}. */
oxc_status oxc_debug_raster_stats(oxc_ctx* ctx, uint32_t* host_out4, void* hip_stream);

/* Test hook: what the last oxc_draw_terrain on this context did (no draw of either kind since); synchronises the stream.
 * out8 = {patches drawn, patches discarded by T2 (an edge factor <= 0 or NaN), list entries skipped by T1 (index out of range), triangles
 * generated (T4's count over the drawn patches), triangles and clipper fan pieces the set-up kept (front-facing, non-zero area),
 * triangles that crossed a clip plane, kept triangles and pieces queued for the big path (pixel box beyond 8 x 8, or the corners' spread
 * at or beyond 4096 units for an unclipped one), fragments that passed the depth range (covered pixels of kept triangles with a depth in
 * (0, 1]: one per atomic maximum issued, on every path -- in-wave boxes, the clipper's lane walks, big list, tiles)}.  The last is counted
 * only after oxc_debug_set_tuning(OXC_TUNE_TERRAIN_DRAW_STATS, 1) (counting instantiations of the kernels, same image, slower); 0 otherwise. */
oxc_status oxc_debug_terrain_draw_stats(oxc_ctx* ctx, uint32_t* host_out8, void* hip_stream);

/* Measurement hook: what the last oxc_draw_physical_pages on this context did; synchronises the stream.
 * out8 = {(triangle, clipmap) pairs whose page box holds a drawable page, fragments written (page and depth tests passed: atomicMin
 * issued), big pairs (pixel box beyond the in-wave path), of those the ones the big list could not hold (drawn again by the overflow
 * pass), (big pair, drawable page) tiles, of those the ones the tile list could not hold (walked by the big pair's wave), pairs that
 * crossed a clip plane, of those the ones the clip queue could not hold (found again by its overflow pass)}.  The first two are counted
 * only after oxc_debug_set_tuning(OXC_TUNE_VSM_DRAW_STATS, 1) (a counting instantiation of the kernels, same image, slower); 0 otherwise. */
oxc_status oxc_debug_vsm_draw_stats(oxc_ctx* ctx, uint32_t* host_out8, void* hip_stream);

/* Measurement hook: what the last oxc_resolve_shadowmap on this context did, counted by a counting instantiation of its kernel (same
 * image, slower) after oxc_debug_set_tuning(OXC_TUNE_VSM_RESOLVE_STATS, 1); synchronises the stream.
 * out8 = {non-sky pixels, taps taken (one per sample position), taps no clipmap served, taps served by clipmap base - 1, by base + 1,
 * pixels that returned the hard-shadow value, the "no blocker" 1.0, the "all blockers" 0.0}. */
oxc_status oxc_debug_vsm_resolve_stats(oxc_ctx* ctx, uint32_t* host_out8, void* hip_stream);

/* Measurement hook: what the last oxc_contact_shadows on this context did, counted by a counting instantiation of its kernel (same
 * image, slower) after oxc_debug_set_tuning(OXC_TUNE_CONTACT_SHADOWS_STATS, 1); synchronises the stream.
 * out12 = {non-sky pixels, depth taps (evaluations of rule 6: one per step taken, five texels each), pixels that found no intersection in
 * their n steps, hits that wrote exactly 0.0, hits that wrote a value strictly inside (0, 1), hits that wrote 1.0, intersections the
 * thickness test rejected, pixels whose n is 2 by the lower clamp (min(steps, u32(floor(length))) < 2), pixels with 2 <= n < steps taken
 * from the ray's length, pixels whose n is steps by the upper clamp (steps >= 2), pixels whose end clip is active (clip < 1.0: the ray
 * is cut at the image border or at z = 0), pixels whose start clip moved the start (max(0.0, m) > 0.0)}. */
oxc_status oxc_debug_contact_shadows_stats(oxc_ctx* ctx, uint32_t* host_out12, void* hip_stream);

/* Measurement hook: what the last oxc_generate_ambient_occlusion on this context did, counted by a counting instantiation of its main kernel
 * (same images, slower) after oxc_debug_set_tuning(OXC_TUNE_AMBIENT_OCCLUSION_STATS, 1); synchronises the stream.
 * out15 = {non-sky pixels, depth samples taken (filtered samples of step 9: two per sample pair, eight texels each), samples whose integer
 * level floor(l) is 0, 1, 2, 3, 4, samples with a non-zero level fraction, non-sky pixels whose stored noisy half is exactly 1.0, strictly
 * inside (0, 1), exactly 0.0, update_sectors calls whose arc has zero width, slices whose sign_norm is -1, 0, +1}. */
oxc_status oxc_debug_ambient_occlusion_stats(oxc_ctx* ctx, uint32_t* host_out15, void* hip_stream);

/* Measurement hook: what the last oxc_decode_visbuffer on this context did, counted by a counting instantiation of its kernel (same
 * images, slower) after oxc_debug_set_tuning(OXC_TUNE_VISBUFFER_DECODE_STATS, 1); synchronises the stream.
 * out4 = {decoded pixels (all four images written from a triangle), empty pixels (rule 1), pixels written as zeros because a vertex index
 * exceeds vertex_count - 1 (rule 2), decoded pixels whose material_index is beyond material_count (the all-zero Material)}. */
oxc_status oxc_debug_visbuffer_decode_stats(oxc_ctx* ctx, uint32_t* host_out4, void* hip_stream);

/* Measurement hook: what the last oxc_decode_visbuffer_textured on this context did, after oxc_debug_set_tuning(
 * OXC_TUNE_VISBUFFER_DECODE_TEXTURED_STATS, 1); synchronises the stream.  out13 = {the four counters of oxc_debug_visbuffer_decode_stats;
 * pixels that sampled their albedo, normal, emissive, metallic-roughness, occlusion image (flag set and the image present, step 13);
 * level taps (two per sampled image under a linear mip filter, one under a nearest one); pixels that sampled a normal image with
 * jacobian_sign == 0; waves with a decoded pixel whose live lanes all named one material (the uniform path), and the other such waves
 * (the per-lane path)}. */
oxc_status oxc_debug_visbuffer_decode_textured_stats(oxc_ctx* ctx, uint32_t* host_out13, void* hip_stream);

/* Measurement hook: what the last oxc_apply_pbr on this context did, counted by a counting instantiation of its kernel (same image,
 * slower) after oxc_debug_set_tuning(OXC_TUNE_PBR_APPLY_STATS, 1); synchronises the stream.
 * out9 = {pixels per outcome class: transparent empty (rule 1), sky (rule 5), fall-through empty (depth == 0.0 with neither flag), lit with
 * NoL > 0, lit with NoL == 0 (rule 11);  light evaluations (one per light per pixel that reaches rule 9) per outcome: skipped by kind,
 * attenuation or intensity out, NdotL out, shaded}. */
oxc_status oxc_debug_pbr_apply_stats(oxc_ctx* ctx, uint32_t* host_out9, void* hip_stream);

/* Measurement hook: what the last oxc_apply_fxaa on this context did, counted by a counting instantiation of its kernel (same image,
 * slower) after oxc_debug_set_tuning(OXC_TUNE_FXAA_STATS, 1); synchronises the stream.
 * out4 = {early-out pixels (rule 4), searched pixels, search taps issued (every Sample at uv1 or uv2 of rule 6: two for the first pair, then
 * one per side not reached per step; the final sample of rule 7 is not one), searched pixels that ran all 12 steps without reaching both
 * ends}. */
oxc_status oxc_debug_fxaa_stats(oxc_ctx* ctx, uint32_t* host_out4, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OXCULL_DEBUG_H */
