// oxcull_raster.hip -- SURVEY 8(f)-2: consumer of cull_geometry's indirect draw (gfx950).
//
// What draw_for_visbuffer does with reordered_indices + the indirect command (Passes/DrawGeometry.cpp:104-190,
// pipeline visbuffer_encode: vs_main passes/visbuffer_encode.slang:24-49, cullMode eBack, depth GreaterOrEqual,
// reversed Z) as a compute rasteriser, so that early cull -> draw -> depth -> generate_hiz -> late cull -> draw can run
// frame after frame without a graphics queue.  The fixed-function rasteriser's exact rules cannot be matched, so
// the rules are stated (include/oxcull.h, oxc_draw_visbuffer) and implemented twice (here and in the CPU checker):
// clipping against w >= 2^-10 and a 64x guard band (round 2: triangles crossing the camera plane used to be dropped), 1/256-pixel snapping, integer edge functions with a top-left rule, z/w interpolated in binary64 from the exact
// edge values, and per pixel the maximum of (depth bits << 32 | vis) through a 64-bit atomic max -- the "R64
// visbuffer" the reference's own note wishes for (visbuffer.slang:43-45), order-independent by construction.
//
// One lane per triangle fetches and sets up.  Triangles whose pixel box is at most kSmallSpan x kSmallSpan (almost all meshlet
// triangles) are rasterised by their wave: the 64 boxes of a wave step are laid end to end (prefix sum of the box sizes) and every
// lane takes one box pixel per iteration, finding its triangle by a binary search over the 64 offsets in LDS -- a lane walking its
// own box made the whole wave wait for the largest box of the 64 (round 1: 0.90 ms for 14.6 M triangles).  Larger
// triangles go to a list that one block per triangle walks.
//
// The rules themselves -- clip planes and clipper, index decode and vertex fetch, row builder, snap and cull mode, pixel box, edge
// functions, top-left rule, depth interpolation, the box-distribution pass -- live in oxcull_raster_device.hpp, shared with the VSM shadow
// draw (oxcull_vsm_draw.hip).  What is the depth|vis image's own and the terrain draw (oxcull_terrain_draw.hip) needs as well -- cullMode
// eBack, the zf > 0 depth test, the 64-bit atomicMax of depth|vis, the push into the segmented big list -- is in
// oxcull_visbuffer_device.hpp.  This file keeps the vertex fetch, the kernels that walk the big list and its 64 x 64 tiles, and the launches.
#include <hip/hip_runtime.h>

#include "oxcull_visbuffer_device.hpp"

#pragma clang fp contract(off)

namespace oxc {

__global__ __launch_bounds__(256) void k_draw_rows(DrawArgs a) { build_draw_rows(a); }

// vs_main (visbuffer_encode.slang:24-49) for the three corners of a triangle given its three index-buffer entries: clip coordinates +
// the encoded vis value.
// first_mli: the MeshletInstance record of idx[0]'s instance when the caller has fetched it already (k_draw_setup, a step ahead).
template <bool PAIR>
OXC_DEV void tri_clip_coords(const DrawArgs& a, const IdxEntry<PAIR> (&idx)[3], float (&clip)[3][4], uint32_t& vis_out, const uint2* first_mli = nullptr) {
  CornerFetch f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t mli_index = entry_instance<PAIR>(a, idx[k]), corner = entry_corner<PAIR>(a, idx[k]);
    float world[3];
    corner_world(a, f, mli_index, corner, k == 0 ? first_mli : nullptr, world);
    mul_mp4(a.pv, world, clip[k]);
    if (k == 0) vis_out = (mli_index << 8) | ((corner / 3u) & 0xFFu);  // VisBufferData(mli, triangle_index / 3).encode()
  }
}

template <bool PAIR>
__global__ __launch_bounds__(256, 5) void k_draw_setup(DrawArgs a) {
  set_half_denorm_flush();
  __shared__ TriLds s_tri[4][64];
  __shared__ uint32_t s_off[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  TriLds* const tl = s_tri[wave];
  uint32_t* const off = s_off[wave];
  // VkDrawIndexedIndirectCommand.indexCount (pairs: a cull call whose index count wrapped zeroed instanceCount, the draw is a no-op)
  const uint32_t tris = (PAIR && a.draw_cmd[1] == 0u) ? 0u : a.draw_cmd[0] / 3u;
  const uint32_t wave_id = blockIdx.x * 4u + (uint32_t)wave, nwaves = gridDim.x * 4u;
  // The fetches of a triangle hang on each other (index -> MeshletInstance -> row -> Meshlet record -> micro index -> vertex id ->
  // position) and the kernel waits for them most of its time: the index entries are fetched two steps ahead and the MeshletInstance
  // record of the first corner one step ahead, which takes the first two links out of a step's own chain.
  IdxEntry<PAIR> nidx[3] = {}, nnidx[3] = {};            // the next / next but one step's index-buffer entries
  uint2 nmli = make_uint2(0u, 0u);                       // the next step's MeshletInstance record (of its first corner)
  if (wave_id * 64u + (uint32_t)lane < tris) {
#pragma unroll
    for (int k = 0; k < 3; k++) nidx[k] = load_entry<PAIR>(a, (wave_id * 64u + (uint32_t)lane) * 3u + (uint32_t)k);
    nmli = reinterpret_cast<const uint2*>(a.meshlet_instances)[entry_instance<PAIR>(a, nidx[0])];
  }
  if ((wave_id + nwaves) * 64u + (uint32_t)lane < tris) {
#pragma unroll
    for (int k = 0; k < 3; k++) nnidx[k] = load_entry<PAIR>(a, ((wave_id + nwaves) * 64u + (uint32_t)lane) * 3u + (uint32_t)k);
  }
  for (uint32_t base = wave_id * 64u; base < tris; base += nwaves * 64u) {  // wave-uniform
    const uint32_t tri = base + (uint32_t)lane;
    const IdxEntry<PAIR> idx[3] = {nidx[0], nidx[1], nidx[2]};
    const uint2 mli0 = nmli;
    {
#pragma unroll
      for (int k = 0; k < 3; k++) nidx[k] = nnidx[k];
      if (tri + nwaves * 64u < tris) nmli = reinterpret_cast<const uint2*>(a.meshlet_instances)[entry_instance<PAIR>(a, nidx[0])];
      const uint32_t nt = tri + 2u * nwaves * 64u;
      if (nt < tris) {
#pragma unroll
        for (int k = 0; k < 3; k++) nnidx[k] = load_entry<PAIR>(a, nt * 3u + (uint32_t)k);
      }
    }
    uint32_t count = 0;  // box pixels this lane's triangle contributes to the wave's small-triangle pass
    if (tri < tris) {
      float clip[3][4];
      uint32_t vis;
      tri_clip_coords<PAIR>(a, idx, clip, vis, &mli0);
      const int cls = tri_clip_class(clip);
      TriSetup t;
      if (cls == 1) {  // rare: crosses the camera plane or the guard band -- clipped by k_draw_clipped, one thread per triangle
        const uint32_t slot = atomicAdd(a.clip_count, 1u);
        if (slot < a.clip_capacity) a.clip_list[slot] = tri;
      } else if (int32_t spread = 0; cls == 0 && tri_finish(a, clip[0], clip[1], clip[2], vis, t, spread)) {
        int32_t px0, py0, px1, py1;
        if (pixel_box(t, (int32_t)a.width, (int32_t)a.height, px0, py0, px1, py1)) {
          const int32_t bw = px1 - px0 + 1, bh = py1 - py0 + 1;
          // (the spread test only fails for triangles reaching far outside the image whose clamped box is small: they take the big path)
          if (bw <= kSmallSpan && bh <= kSmallSpan && spread < 4096) {
            count = (uint32_t)(bw * bh);
            TriLds o;
#pragma unroll
            for (int k = 0; k < 3; k++) o.x[k] = t.x[k], o.y[k] = t.y[k], o.z[k] = t.z[k];
            o.vis = t.vis;
            pack_small(t, px0, py0, bw, o);
            tl[lane] = o;
          } else {
            push_big(a, t, wave_id % kBigSegs);
          }
        }
      }
    }
    wave_small_boxes(tl, off, count, lane, [&](const TriLds& q, int32_t e0, int32_t e1, int32_t e2, double inv_area, uint32_t px, uint32_t py) {
      fragment(e0, e1, e2, q.z[0], q.z[1], q.z[2], inv_area, q.vis, px, py, a.width, a.visdepth);
    });
  }
}

// The clipper (clip_polygon), fan triangulation, then the same setup as an unclipped triangle.
// RESCAN: the overflow pass.  More triangles crossed a clip plane than the id queue holds (clip_capacity): the ids beyond it were
// not recorded, so this instantiation walks the whole index list again and clips every crossing triangle it finds.  Drawing a
// triangle twice leaves the image unchanged (per-pixel maximum), so no bookkeeping of which ones the queue did hold is needed.
// It returns at once when the queue did not overflow.
template <bool RESCAN, bool PAIR>
__global__ __launch_bounds__(64) void k_draw_clipped(DrawArgs a) {
  set_half_denorm_flush();
  if (RESCAN && *a.clip_count <= a.clip_capacity) return;
  const uint32_t count = RESCAN ? ((PAIR && a.draw_cmd[1] == 0u) ? 0u : a.draw_cmd[0] / 3u) : min(*a.clip_count, a.clip_capacity);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    float clip[3][4];
    uint32_t vis;
    const uint32_t tri = RESCAN ? i : a.clip_list[i];
    const IdxEntry<PAIR> idx[3] = {load_entry<PAIR>(a, tri * 3u), load_entry<PAIR>(a, tri * 3u + 1u), load_entry<PAIR>(a, tri * 3u + 2u)};
    tri_clip_coords<PAIR>(a, idx, clip, vis);
    if (RESCAN && tri_clip_class(clip) != 1) continue;
    float poly[2][9][4];
    for (int k = 0; k < 3; k++)
      for (int c = 0; c < 4; c++) poly[0][k][c] = clip[k][c];
    int cur;
    const int n = clip_polygon(poly, cur);
    for (int k = 1; k + 1 < n; k++) {
      TriSetup t;
      int32_t spread;
      if (tri_finish(a, poly[cur][0], poly[cur][k], poly[cur][k + 1], vis, t, spread)) tri_emit(a, t, blockIdx.x % kBigSegs);
    }
  }
}

// A pixel rectangle of a big triangle's box, walked by a wave in 8 x 8 pixel blocks (lane = pixel of the block), 64-bit edge functions.
OXC_DEV void raster_rect64(const DrawArgs& a, const TriRaster& r, int64_t ox, int64_t oy, int64_t x1, int64_t y1, int lane, uint32_t* tally = nullptr) {
  for (int64_t by = oy; by <= y1; by += 8)
    for (int64_t bx = ox; bx <= x1; bx += 8) {
      const int64_t px = bx + (lane & 7), py = by + (lane >> 3);
      if (px <= x1 && py <= y1) {
        int64_t e0, e1, e2;
        tri_edges(r, px, py, e0, e1, e2);
        tri_fragment(r, e0, e1, e2, px, py, a.width, a.visdepth, tally);
      }
    }
}
// The same with 32-bit edge functions when they are exact for this rectangle (wave-uniform test).
OXC_DEV void raster_rect(const DrawArgs& a, const TriRaster& r, int64_t ox, int64_t oy, int64_t x1, int64_t y1, int lane, uint32_t* tally = nullptr) {
  // every difference the edge functions of this rectangle see: corner - corner, pixel centre - corner
  const int64_t cx0 = ox * 256 + 128, cx1 = x1 * 256 + 128, cy0 = oy * 256 + 128, cy1 = y1 * 256 + 128;
  const int64_t lox = min(min(min(r.X[0], r.X[1]), r.X[2]), cx0), hix = max(max(max(r.X[0], r.X[1]), r.X[2]), cx1);
  const int64_t loy = min(min(min(r.Y[0], r.Y[1]), r.Y[2]), cy0), hiy = max(max(max(r.Y[0], r.Y[1]), r.Y[2]), cy1);
  if (hix - lox < 32768 && hiy - loy < 32768) {
    const int32_t X0 = (int32_t)r.X[0], X1 = (int32_t)r.X[1], X2 = (int32_t)r.X[2], Y0 = (int32_t)r.Y[0], Y1 = (int32_t)r.Y[1], Y2 = (int32_t)r.Y[2];
    for (int32_t by = (int32_t)oy; by <= (int32_t)y1; by += 8)
      for (int32_t bx = (int32_t)ox; bx <= (int32_t)x1; bx += 8) {
        const int32_t px = bx + (lane & 7), py = by + (lane >> 3);
        if (px <= (int32_t)x1 && py <= (int32_t)y1) {
          const int32_t cx = px * 256 + 128, cy = py * 256 + 128;
          const int32_t e0 = edge_fn32(X1, Y1, X2, Y2, cx, cy), e1 = edge_fn32(X2, Y2, X0, Y0, cx, cy), e2 = edge_fn32(X0, Y0, X1, Y1, cx, cy);
          if (covered(e0, e1, e2, (int32_t)r.b0, (int32_t)r.b1, (int32_t)r.b2))
            fragment(e0, e1, e2, r.z[0], r.z[1], r.z[2], r.inv_area, r.vis, (uint32_t)px, (uint32_t)py, a.width, a.visdepth, tally);
        }
      }
  } else {
    raster_rect64(a, r, ox, oy, x1, y1, lane, tally);
  }
}

// One wave per big triangle.  Round 1 gave every big triangle a 256-thread block: 0.43 ms for the 330 K triangles of the loop
// benchmark whose boxes are barely larger than 8 x 8, and a full-screen triangle was a single block's 16 K iterations.  Here a box of
// at most 64 x 64 pixels (nearly all) is walked at once; a larger one is cut into 64 x 64 tiles that go to the tile list
// (k_draw_big_tiles: one wave per tile), so a screen-filling triangle becomes a thousand balanced items.
__global__ __launch_bounds__(256) void k_draw_big(DrawArgs a) {
#define OXC_BIG_PART 1
#define OXC_BIG_TALLY nullptr
#include "oxcull_draw_big.inc"
#undef OXC_BIG_TALLY
#undef OXC_BIG_PART
}


// One wave per tile-list item: a 64 x 64 pixel tile of a triangle whose box is larger than that.
__global__ __launch_bounds__(256) void k_draw_big_tiles(DrawArgs a) {
#define OXC_BIG_PART 2
#define OXC_BIG_TALLY nullptr
#include "oxcull_draw_big.inc"
#undef OXC_BIG_TALLY
#undef OXC_BIG_PART
}

// The counting instantiations of the two, for a draw that reports its fragments (oxc_draw_terrain with OXC_TUNE_TERRAIN_DRAW_STATS): every
// lane counts the fragments of its pixels that passed the depth range, a wave adds its sum to *fragments.  Same image.
OXC_DEV void add_wave_tally(uint32_t tally, uint32_t* fragments) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) tally += __shfl_xor(tally, o, 64);
  if ((threadIdx.x & 63) == 0 && tally) atomicAdd(fragments, tally);
}
__global__ __launch_bounds__(256) void k_draw_big_count(DrawArgs a, uint32_t* fragments) {
  uint32_t tally = 0;
  {
#define OXC_BIG_PART 1
#define OXC_BIG_TALLY (&tally)
#include "oxcull_draw_big.inc"
#undef OXC_BIG_TALLY
#undef OXC_BIG_PART
  }
  add_wave_tally(tally, fragments);
}
__global__ __launch_bounds__(256) void k_draw_big_tiles_count(DrawArgs a, uint32_t* fragments) {
  uint32_t tally = 0;
  {
#define OXC_BIG_PART 2
#define OXC_BIG_TALLY (&tally)
#include "oxcull_draw_big.inc"
#undef OXC_BIG_TALLY
#undef OXC_BIG_PART
  }
  add_wave_tally(tally, fragments);
}

// The draw's clears as one kernel: `n` texels of the packed image and `words` u32 of the scratch header.  Not hipMemsetAsync: captured into
// a HIP graph, the memset node of the image zero-filled it on the first replay only and wrote other bytes from the second replay on
// (DESIGN.md section 15); a kernel node replays as it was captured.
__global__ __launch_bounds__(256) void k_draw_clear(unsigned long long* __restrict__ visdepth, uint64_t n, uint32_t* __restrict__ header, uint32_t words) {
  const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = first; i < n; i += stride) visdepth[i] = 0ull;
  for (uint64_t i = first; i < words; i += stride) header[i] = 0u;
}

__global__ __launch_bounds__(256) void k_resolve_visbuffer(const unsigned long long* __restrict__ visdepth, uint64_t n, float* __restrict__ depth,
                                                           uint32_t* __restrict__ vis) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long v = visdepth[i];
    if (depth) depth[i] = asf((uint32_t)(v >> 32));
    if (vis) vis[i] = (uint32_t)v;
  }
}

// The three launches around a draw's own kernels, also taken by oxc_draw_terrain (oxcull_terrain_draw.hip), whose triangles go through the
// same big list and tiles: the clears, the big list with its tiles, the optional resolve.
void launch_draw_clear(const DrawArgs& a, bool clear, uint32_t max_grid, hipStream_t s) {
  const uint64_t n = (uint64_t)a.width * a.height;
  // the image (with `clear`) and the clip / tile counters and the big list's segment counters
  hipLaunchKernelGGL(k_draw_clear, dim3((uint32_t)std::min<uint64_t>(((clear ? n : 0) + kRasterHeaderBytes / 4u + 255) / 256, max_grid)), dim3(256), 0, s,
                     a.visdepth, clear ? n : 0, a.clip_count, kRasterHeaderBytes / 4u);
}
void launch_draw_big(const DrawArgs& a, uint32_t max_grid, hipStream_t s, uint32_t* fragments) {
  if (fragments) {
    hipLaunchKernelGGL(k_draw_big_count, dim3(max_grid), dim3(256), 0, s, a, fragments);
    hipLaunchKernelGGL(k_draw_big_tiles_count, dim3(max_grid), dim3(256), 0, s, a, fragments);
    return;
  }
  hipLaunchKernelGGL(k_draw_big, dim3(max_grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_draw_big_tiles, dim3(max_grid), dim3(256), 0, s, a);
}
void launch_resolve_visbuffer(const DrawArgs& a, float* depth_out, uint32_t* vis_out, uint32_t max_grid, hipStream_t s) {
  const uint64_t n = (uint64_t)a.width * a.height;
  if (depth_out || vis_out)
    hipLaunchKernelGGL(k_resolve_visbuffer, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, max_grid)), dim3(256), 0, s, a.visdepth, n, depth_out, vis_out);
}

void launch_draw_visbuffer(const DrawArgs& a, bool clear, float* depth_out, uint32_t* vis_out, uint32_t max_grid, hipStream_t s) {
  launch_draw_clear(a, clear, max_grid, s);
  hipLaunchKernelGGL(k_draw_rows, dim3(std::max(1u, std::min((a.mesh_instance_count + 255u) / 256u, max_grid))), dim3(256), 0, s, a);
  if (a.wide == 2u) {  // {id, corner} pairs
    hipLaunchKernelGGL(k_draw_setup<true>, dim3(max_grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_draw_clipped<false, true>), dim3(std::min(256u, max_grid)), dim3(64), 0, s, a);
    hipLaunchKernelGGL((k_draw_clipped<true, true>), dim3(max_grid), dim3(64), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_draw_setup<false>, dim3(max_grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_draw_clipped<false, false>), dim3(std::min(256u, max_grid)), dim3(64), 0, s, a);
    hipLaunchKernelGGL((k_draw_clipped<true, false>), dim3(max_grid), dim3(64), 0, s, a);  // (returns at once unless the id queue overflowed)
  }
  launch_draw_big(a, max_grid, s);
  launch_resolve_visbuffer(a, depth_out, vis_out, max_grid, s);
}

}  // namespace oxc
