// oxcull_terrain_draw.hip -- the tessellated terrain draw into the depth|vis image (gfx950): RendererInstance::draw_terrain_for_visbuffer
// (Passes/Terrain.cpp:218-277, pipeline terrain_visbuffer, passes/terrain_visbuffer.slang) as a compute pass.  Rules: include/oxcull.h,
// oxc_draw_terrain (steps T1 - T7); design: DESIGN.md section 30.
//
//   k_terrain_draw   a block of 256 threads takes a visible patch, with a stride loop over the list whose length it reads from the
//                    draw command.  Threads 0 - 3 evaluate the corners (T1) and the edge factors (T2); every thread then derives the six
//                    segment counts and the block lays the six parameter lists (T3) into LDS.  The patch is drawn in phases, each one a
//                    set of domain points evaluated ONCE into LDS as clip coordinates (T5: two lerps and one heightmap bilinear per
//                    point, not per triangle corner) and the triangles that index them (T4): the inner grid in tiles of at most 16 x 16
//                    cells (17 x 17 points), then the four ring strips (their merge order is written by one thread: at most 124 steps).
//                    A lane takes a triangle: clip class, cullMode eBack set-up, pixel box.  Boxes up to 8 x 8 go through the wave's
//                    box-distribution pass, larger ones into the segmented big list that k_draw_big / k_draw_big_tiles of
//                    oxcull_raster.hip walk afterwards; a triangle that crosses a clip plane is clipped by its lane (rare).
//
//                    k_terrain_draw<true> is the counting instantiation (OXC_TUNE_TERRAIN_DRAW_STATS): it also tallies the fragments that
//                    pass the depth range; the big list is then walked by k_draw_big_count / k_draw_big_tiles_count.
//
// Everything behind "three clip-space corners" is oxcull_raster_device.hpp / oxcull_visbuffer_device.hpp, the code oxc_draw_visbuffer runs.
#include <hip/hip_runtime.h>

#include "oxcull_terrain_device.hpp"
#include "oxcull_visbuffer_device.hpp"

#pragma clang fp contract(off)

namespace oxc {
namespace {

constexpr uint32_t kTerrainVis = 0xFFFFFE00u;  // VisBufferData(TERRAIN_INSTANCE_ID, 0).encode()
constexpr int kTileCells = 16;                 // cells a side of an inner-grid tile
constexpr int kTilePoints = (kTileCells + 1) * (kTileCells + 1);
constexpr int kRingInner = 64;                 // a ring strip's inner points follow its outer points at this index
constexpr int kMaxRingTris = 63 + 61;
static_assert(kRingInner + 62 <= kTilePoints, "a ring strip's points fit the tile's rows");

// T3 for one factor: the clamped factor -> segment count
OXC_DEV float clamp_factor(float f) { return fminf(fmaxf(f, 1.0f), 63.0f); }
OXC_DEV int segments_of(float fc) {
  const int c = (int)ceilf(fc);  // 1 .. 63
  return c | 1;                  // the smallest odd integer >= fc
}
// t_k of the list with clamped factor fc and n segments
OXC_DEV float param_at(float fc, int n, int k) {
  if (k <= 0) return 0.0f;
  if (k >= n) return 1.0f;
  const float r = 1.0f / fc;
  const float s = (1.0f - (float)(n - 2) * r) * 0.5f;
  const int h = (n - 1) / 2;
  if (k <= h) return s + (float)(k - 1) * r;
  return 1.0f - (s + (float)(n - k - 1) * r);
}

// B3 on the draw's heightmap
OXC_DEV float sample_height(const TerrainDrawArgs& a, float wx, float wz) {
  const oxc_terrain_data& T = a.t;
  const float u = (wx - T.world_min[0]) * T.inv_world_size[0], v = (wz - T.world_min[1]) * T.inv_world_size[1];
  const MapTaps t = map_taps(u, v, a.map_w, a.map_h);
  const float t00 = (float)a.heightmap[t.r0 + t.ax.i0] / 65535.0f, t10 = (float)a.heightmap[t.r0 + t.ax.i1] / 65535.0f;
  const float t01 = (float)a.heightmap[t.r1 + t.ax.i0] / 65535.0f, t11 = (float)a.heightmap[t.r1 + t.ax.i1] / 65535.0f;
  const float n = lerp_f(lerp_f(t00, t10, t.ax.f), lerp_f(t01, t11, t.ax.f), t.ay.f);
  return T.base_height + n * T.height_scale;
}

OXC_DEV float distance3(const float* p, const float* q) {
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// T2: edge_tessellation
OXC_DEV float edge_factor(const TerrainDrawArgs& a, const float* p0, const float* p1) {
  const float center[3] = {(p0[0] + p1[0]) * 0.5f, (p0[1] + p1[1]) * 0.5f, (p0[2] + p1[2]) * 0.5f};
  const float radius = distance3(p0, p1) * 0.5f;
  const float view_distance = fmaxf(distance3(center, a.camera_position) - radius, a.near_clip);
  const float projected_pixels = ((2.0f * radius) * a.projection_scale) / view_distance;
  return fminf(fmaxf(projected_pixels / a.t.target_edge_pixels, 1.0f), a.t.max_tessellation);
}

// T5: lerp with the stated deviation -- a coordinate that is exactly 0 or 1 selects the operand itself
OXC_DEV float lerp_end(float p, float q, float t) { return t == 0.0f ? p : (t == 1.0f ? q : p + (q - p) * t); }

struct PatchLds {
  float corner[4][3];  // world positions of (0,0), (1,0), (1,1), (0,1)
  float factor[4];     // edge factors 0 .. 3
  float list[6][64];   // parameter lists: 0 .. 3 the outer edges, 4 the inner u axis, 5 the inner v axis
  float4 pts[kTilePoints];
  uint8_t ring[kMaxRingTris][4];
  uint32_t ring_count;
};

// T5 for the domain point (u, v) of the block's patch: clip coordinates
OXC_DEV float4 domain_point(const TerrainDrawArgs& a, const PatchLds& P, float u, float v) {
  const float ax = lerp_end(P.corner[0][0], P.corner[1][0], u), az = lerp_end(P.corner[0][2], P.corner[1][2], u);
  const float bx = lerp_end(P.corner[3][0], P.corner[2][0], u), bz = lerp_end(P.corner[3][2], P.corner[2][2], u);
  const float x = lerp_end(ax, bx, v), z = lerp_end(az, bz, v);
  const float world[3] = {x, sample_height(a, x, z), z};
  float clip[4];
  mul_mp4(a.r.pv, world, clip);
  return make_float4(clip[0], clip[1], clip[2], clip[3]);
}

struct Tally {
  uint32_t setup = 0, clipped = 0, big = 0, fragments = 0;
};

// T6 + T7 for the wave's next 64 triangles of the current phase: lane's triangle (i0, i1, i2), counter-clockwise in (u, v); valid false
// for the lanes past the phase's end.  The single global exchange of T6 hands (i0, i2, i1) to the set-up.  COUNT: the counting instantiation,
// which also tallies the fragments that pass the depth range on every path the lane itself walks.
template <bool COUNT>
OXC_DEV void wave_triangles(const TerrainDrawArgs& a, const PatchLds& P, bool valid, uint32_t i0, uint32_t i1, uint32_t i2, TriLds* tl, uint32_t* off, int lane, uint32_t seg,
                            Tally& tally) {
  uint32_t count = 0;
  uint32_t* const frags = COUNT ? &tally.fragments : nullptr;
  if (valid) {
    const float4 q0 = P.pts[i0], q1 = P.pts[i2], q2 = P.pts[i1];
    const float clip[3][4] = {{q0.x, q0.y, q0.z, q0.w}, {q1.x, q1.y, q1.z, q1.w}, {q2.x, q2.y, q2.z, q2.w}};
    const int cls = tri_clip_class(clip);
    TriSetup t;
    if (cls == 1) {  // rare: crosses the camera plane or the guard band -- clipped here, fanned, every piece as tri_emit takes it
      tally.clipped++;
      float poly[2][9][4];
      for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) poly[0][k][c] = clip[k][c];
      int cur;
      const int n = clip_polygon(poly, cur);
      for (int k = 1; k + 1 < n; k++) {
        int32_t spread;
        if (tri_finish(a.r, poly[cur][0], poly[cur][k], poly[cur][k + 1], kTerrainVis, t, spread)) {
          tally.setup++;
          int32_t px0, py0, px1, py1;
          if (pixel_box(t, (int32_t)a.r.width, (int32_t)a.r.height, px0, py0, px1, py1) && !((px1 - px0) < kSmallSpan && (py1 - py0) < kSmallSpan)) tally.big++;
          tri_emit(a.r, t, seg, frags);
        }
      }
    } else if (int32_t spread = 0; cls == 0 && tri_finish(a.r, clip[0], clip[1], clip[2], kTerrainVis, t, spread)) {
      tally.setup++;
      int32_t px0, py0, px1, py1;
      if (pixel_box(t, (int32_t)a.r.width, (int32_t)a.r.height, px0, py0, px1, py1)) {
        const int32_t bw = px1 - px0 + 1, bh = py1 - py0 + 1;
        if (bw <= kSmallSpan && bh <= kSmallSpan && spread < 4096) {
          count = (uint32_t)(bw * bh);
          TriLds o;
#pragma unroll
          for (int k = 0; k < 3; k++) o.x[k] = t.x[k], o.y[k] = t.y[k], o.z[k] = t.z[k];
          o.vis = t.vis;
          pack_small(t, px0, py0, bw, o);
          tl[lane] = o;
        } else {
          tally.big++;
          push_big(a.r, t, seg, frags);
        }
      }
    }
  }
  wave_small_boxes(tl, off, count, lane, [&](const TriLds& q, int32_t e0, int32_t e1, int32_t e2, double inv_area, uint32_t px, uint32_t py) {
    fragment(e0, e1, e2, q.z[0], q.z[1], q.z[2], inv_area, q.vis, px, py, a.r.width, a.r.visdepth, frags);
  });
}

OXC_DEV uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace

template <bool COUNT>
__global__ __launch_bounds__(256) void k_terrain_draw(TerrainDrawArgs a) {
  __shared__ PatchLds P;
  __shared__ TriLds s_tri[4][64];
  __shared__ uint32_t s_off[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  TriLds* const tl = s_tri[wave];
  uint32_t* const off = s_off[wave];
  const uint32_t seg = (blockIdx.x * 4u + (uint32_t)wave) % kBigSegs;
  const oxc_terrain_data& T = a.t;
  const uint32_t instance_count = a.draw_cmd[1], first_instance = a.draw_cmd[3];  // VkDrawIndirectCommand; words 0 and 2 are not read
  const uint64_t patches = (uint64_t)T.patch_count[0] * T.patch_count[1];
  Tally tally;
  uint32_t drawn = 0, discarded = 0, skipped = 0, generated = 0;  // kept by thread 0

  // The entries at or past the list's end are skipped in one step, so a garbage command costs nothing and the loop's bound cannot wrap:
  // listed <= visible_capacity <= 2^24 (patch_count is at most 4096 a side; the host clamps the capacity to that).
  const uint64_t room = first_instance < a.visible_capacity ? a.visible_capacity - first_instance : 0ull;
  const uint32_t listed = (uint32_t)(instance_count < room ? instance_count : room);
  if (blockIdx.x == 0 && tid == 0) skipped = instance_count - listed;

  for (uint32_t item = blockIdx.x; item < listed; item += gridDim.x) {  // block-uniform
    // ---- T1: the patch and its corners ----
    const uint32_t patch_index = a.visible[(uint64_t)first_instance + item];
    if (patch_index >= patches) {
      if (tid == 0) skipped++;
      continue;
    }
    __syncthreads();  // the previous patch's phases have read P
    if (tid < 4) {
      const uint32_t px = patch_index % T.patch_count[0] + ((tid == 1 || tid == 2) ? 1u : 0u), pz = patch_index / T.patch_count[0] + (tid >= 2 ? 1u : 0u);
      const float gx = (float)px / (float)T.patch_count[0], gz = (float)pz / (float)T.patch_count[1];
      const float wx = T.world_min[0] + gx * T.world_size[0], wz = T.world_min[1] + gz * T.world_size[1];
      P.corner[tid][0] = wx, P.corner[tid][1] = sample_height(a, wx, wz), P.corner[tid][2] = wz;
    }
    __syncthreads();
    // ---- T2: edges 0: (p0, p3), 1: (p0, p1), 2: (p1, p2), 3: (p3, p2) ----
    if (tid < 4) {
      const int ea[4] = {0, 0, 1, 3}, eb[4] = {3, 1, 2, 2};
      P.factor[tid] = edge_factor(a, P.corner[ea[tid]], P.corner[eb[tid]]);
    }
    __syncthreads();
    const float e0 = P.factor[0], e1 = P.factor[1], e2 = P.factor[2], e3 = P.factor[3];
    if (!(e0 > 0.0f) || !(e1 > 0.0f) || !(e2 > 0.0f) || !(e3 > 0.0f)) {  // Vulkan: a factor <= 0 or NaN discards the patch
      if (tid == 0) discarded++;
      continue;
    }
    // ---- T3, T4: the six lists (every thread the same values) ----
    float fc[6] = {clamp_factor(e0), clamp_factor(e1), clamp_factor(e2), clamp_factor(e3), clamp_factor(fmaxf(e1, e3)), clamp_factor(fmaxf(e0, e2))};
    int n[6];
#pragma unroll
    for (int l = 0; l < 6; l++) n[l] = segments_of(fc[l]);
    const bool all_one = n[0] == 1 && n[1] == 1 && n[2] == 1 && n[3] == 1 && n[4] == 1 && n[5] == 1;
    if (!all_one) {
#pragma unroll
      for (int l = 4; l < 6; l++)
        if (n[l] == 1) fc[l] = asf(0x3F800001u), n[l] = 3;
    }
    for (int idx = tid; idx < 6 * 64; idx += 256) {
      const int l = idx >> 6, k = idx & 63;
      float f = fc[0];
      int nn = n[0];
#pragma unroll
      for (int q = 1; q < 6; q++)
        if (l == q) f = fc[q], nn = n[q];
      if (k <= nn) P.list[l][k] = param_at(f, nn, k);
    }
    const int nu = n[4], nv = n[5];
    if (tid == 0) {
      drawn++;
      generated += all_one ? 2u : (uint32_t)(2 * (nu - 2) * (nv - 2) + (n[0] + nv - 2) + (n[2] + nv - 2) + (n[1] + nu - 2) + (n[3] + nu - 2));
    }
    __syncthreads();

    if (all_one) {  // two triangles over the corners, split along (0,0) - (1,1)
      if (tid < 4) P.pts[tid] = domain_point(a, P, (tid == 1 || tid == 2) ? 1.0f : 0.0f, tid >= 2 ? 1.0f : 0.0f);
      __syncthreads();
      if (wave == 0) wave_triangles<COUNT>(a, P, lane < 2, 0u, lane == 0 ? 1u : 2u, lane == 0 ? 2u : 3u, tl, off, lane, seg, tally);
      continue;
    }

    // ---- the inner grid (U_i, V_j), 1 <= i <= nu - 1, 1 <= j <= nv - 1, in tiles ----
    for (int j0 = 1; j0 < nv - 1; j0 += kTileCells)
      for (int i0 = 1; i0 < nu - 1; i0 += kTileCells) {
        const int pw = min(kTileCells, nu - 1 - i0) + 1, ph = min(kTileCells, nv - 1 - j0) + 1;  // points a side
        __syncthreads();  // the previous phase has read P.pts
        for (int p = tid; p < pw * ph; p += 256) P.pts[p] = domain_point(a, P, P.list[4][i0 + p % pw], P.list[5][j0 + p / pw]);
        __syncthreads();
        const uint32_t ntri = (uint32_t)(2 * (pw - 1) * (ph - 1));
        for (uint32_t base = (uint32_t)wave * 64u; base < ntri; base += 256u) {  // wave-uniform
          const uint32_t t = base + (uint32_t)lane, cell = t >> 1;
          const uint32_t cx = cell % (uint32_t)(pw - 1), cy = cell / (uint32_t)(pw - 1);
          const uint32_t p00 = cy * (uint32_t)pw + cx, p10 = p00 + 1u, p01 = p00 + (uint32_t)pw, p11 = p01 + 1u;
          wave_triangles<COUNT>(a, P, t < ntri, p00, (t & 1u) ? p11 : p10, (t & 1u) ? p01 : p11, tl, off, lane, seg, tally);
        }
      }

    // ---- the four ring strips: side 0: u = 0 (edge 0), 1: v = 0 (edge 1), 2: u = 1 (edge 2), 3: v = 1 (edge 3) ----
    for (int side = 0; side < 4; side++) {
      const bool along_v = (side & 1) == 0;            // the strip's parameter is v (sides 0, 2) or u (sides 1, 3)
      const int no = n[side], axis = along_v ? 5 : 4;  // outer segments; the inner list is the axis list without its two ends
      const int ni = (along_v ? nv : nu) - 2;          // inner segments
      const float fixed_outer = side >= 2 ? 1.0f : 0.0f;
      const float fixed_inner = P.list[along_v ? 4 : 5][side >= 2 ? (along_v ? nu : nv) - 1 : 1];
      __syncthreads();  // the previous phase has read P.pts and P.ring
      for (int p = tid; p < no + 1 + ni + 1; p += 256) {
        const bool outer = p <= no;
        const float t = outer ? P.list[side][p] : P.list[axis][p - no], other = outer ? fixed_outer : fixed_inner;
        P.pts[outer ? p : kRingInner + (p - no - 1)] = along_v ? domain_point(a, P, other, t) : domain_point(a, P, t, other);
      }
      if (tid == 0) {  // the merge of the two sorted lists
        int oa = 0, ib = 0;
        uint32_t m = 0;
        const bool flip = side == 1 || side == 2;  // these two constructions come out clockwise in (u, v)
        while (oa < no || ib < ni) {
          const bool step_outer = ib == ni || (oa < no && P.list[side][oa + 1] <= P.list[axis][ib + 2]);
          const uint32_t c0 = (uint32_t)oa, c1 = (uint32_t)(kRingInner + ib), c2 = step_outer ? (uint32_t)(oa + 1) : (uint32_t)(kRingInner + ib + 1);
          P.ring[m][0] = (uint8_t)c0, P.ring[m][1] = (uint8_t)(flip ? c2 : c1), P.ring[m][2] = (uint8_t)(flip ? c1 : c2);
          m++;
          if (step_outer) oa++; else ib++;
        }
        P.ring_count = m;
      }
      __syncthreads();
      const uint32_t ntri = P.ring_count;
      for (uint32_t base = (uint32_t)wave * 64u; base < ntri; base += 256u) {  // wave-uniform
        const uint32_t t = min(base + (uint32_t)lane, ntri - 1u);
        wave_triangles<COUNT>(a, P, base + (uint32_t)lane < ntri, P.ring[t][0], P.ring[t][1], P.ring[t][2], tl, off, lane, seg, tally);
      }
    }
  }

  // the counters of oxc_debug_terrain_draw_stats: one atomic per wave and counter
  const uint32_t sums[3] = {wave_sum(tally.setup), wave_sum(tally.clipped), wave_sum(tally.big)};
  if (COUNT) {
    const uint32_t f = wave_sum(tally.fragments);
    if (lane == 0 && f) atomicAdd(a.stats + 7, f);
  }
  if (lane == 0) {
    if (sums[0]) atomicAdd(a.stats + 4, sums[0]);
    if (sums[1]) atomicAdd(a.stats + 5, sums[1]);
    if (sums[2]) atomicAdd(a.stats + 6, sums[2]);
  }
  if (tid == 0) {
    if (drawn) atomicAdd(a.stats + 0, drawn);
    if (discarded) atomicAdd(a.stats + 1, discarded);
    if (skipped) atomicAdd(a.stats + 2, skipped);
    if (generated) atomicAdd(a.stats + 3, generated);
  }
}

void launch_draw_terrain(const TerrainDrawArgs& a, bool clear, bool count_fragments, float* depth_out, uint32_t* vis_out, uint32_t max_grid, hipStream_t s) {
  launch_draw_clear(a.r, clear, max_grid, s);  // also zeroes the header, where the counters live
  if (count_fragments)
    hipLaunchKernelGGL(k_terrain_draw<true>, dim3(max_grid), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_terrain_draw<false>, dim3(max_grid), dim3(256), 0, s, a);
  launch_draw_big(a.r, max_grid, s, count_fragments ? a.stats + 7 : nullptr);
  launch_resolve_visbuffer(a.r, depth_out, vis_out, max_grid, s);
}

}  // namespace oxc
