// oxcull_terrain_brush.hip -- the terrain brush (gfx950): the two compute passes of RendererInstance::apply_terrain_brush
// (Passes/Terrain.cpp:35-132): passes/terrain_brush_trace.slang and passes/terrain_brush_apply.slang.  Rules: include/oxcull.h,
// oxc_apply_terrain_brush (steps B1 - B10); design: DESIGN.md section 25.
//
//   k_terrain_brush_trace   one block of 256 threads.  The reference marches with one thread: 513 bilinear taps, each waiting for its loads.
//                           No gap of the march depends on an earlier one, so here thread t takes the gaps t and t + 256 (thread 0 also
//                           gap 512) and leaves them in LDS.  After one barrier thread t tests the crossings t + 1 and t + 257; a wave's
//                           smallest comes from a ballot and its first set bit, the block's from four LDS entries.  Wave 0 then runs the 24
//                           bisection steps, every lane the same values, and lane 0 writes the two records.  The direction and the span are
//                           evaluated by every thread: the same operations on the same kernel arguments.
//   k_terrain_brush_apply   one texel per lane, an 8 x 8 tile per wave, 16 x 16 per block: the reference's work group.  The hit record is
//                           loaded through a uniform address once per wave; the mode is a kernel argument, so its branch is uniform.
//                           Smooth reads its 25 texels directly: neighbouring lanes read overlapping rows of a 2-byte image, which the
//                           cache serves.
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_terrain_device.hpp"

namespace oxc {
namespace {
constexpr uint32_t kMarchSteps = 512, kRefineSteps = 24;
constexpr uint32_t kNoCrossing = 0xFFFFFFFFu;

// the unorm16 load of texel (x, y) clamped to the map per axis: load_height of terrain_brush_apply.slang
OXC_DEV float load_height(const TerrainBrushArgs& a, int x, int y) {
  const int cx = clamp_i(x, 0, (int)a.p.resolution[0] - 1), cy = clamp_i(y, 0, (int)a.p.resolution[1] - 1);
  return (float)a.heightmap[(size_t)cy * a.p.resolution[0] + cx] / 65535.0f;
}

// B3
OXC_DEV float sample_height(const TerrainBrushArgs& a, float wx, float wz) {
  const oxc_terrain_brush_params& B = a.p;
  const uint32_t w = B.resolution[0], h = B.resolution[1];
  const float u = (wx - B.world_min[0]) * B.inv_world_size[0], v = (wz - B.world_min[1]) * B.inv_world_size[1];
  const MapTaps t = map_taps(u, v, w, h);
  const float t00 = (float)a.heightmap[t.r0 + t.ax.i0] / 65535.0f, t10 = (float)a.heightmap[t.r0 + t.ax.i1] / 65535.0f;
  const float t01 = (float)a.heightmap[t.r1 + t.ax.i0] / 65535.0f, t11 = (float)a.heightmap[t.r1 + t.ax.i1] / 65535.0f;
  const float n = lerp_f(lerp_f(t00, t10, t.ax.f), lerp_f(t01, t11, t.ax.f), t.ay.f);
  return B.base_height + n * B.height_scale;
}

// B4: the gap at ray parameter t
OXC_DEV float gap_at(const TerrainBrushArgs& a, const V3& d, float t) {
  const oxc_terrain_brush_params& B = a.p;
  const float px = B.ray_origin[0] + d.x * t, py = B.ray_origin[1] + d.y * t, pz = B.ray_origin[2] + d.z * t;
  return py - sample_height(a, px, pz);
}

// B2: false when the axis ends the clip with the span (1, 0)
OXC_DEV bool clip_axis(float o, float d, float lo, float hi, float& near, float& far) {
  if (__builtin_fabsf(d) < 1e-6f) return !(o < lo || o > hi);
  const float t0 = (lo - o) / d, t1 = (hi - o) / d;
  near = fmaxf(near, fminf(t0, t1));
  far = fminf(far, fmaxf(t0, t1));
  return true;
}

// B1 - B6
__global__ __launch_bounds__(256) void k_terrain_brush_trace(TerrainBrushArgs a) {
  __shared__ float gaps[kMarchSteps + 1];
  __shared__ uint32_t wave_first[4];
  const oxc_terrain_brush_params& B = a.p;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

  const V3 d = normalize3({B.ray_direction[0], B.ray_direction[1], B.ray_direction[2]});
  float near = 0.0f, far = 1e9f;
  const bool inside = clip_axis(B.ray_origin[0], d.x, B.world_min[0], B.world_min[0] + B.world_size[0], near, far) &&
                      clip_axis(B.ray_origin[2], d.z, B.world_min[1], B.world_min[1] + B.world_size[1], near, far);
  const float span_x = inside ? near : 1.0f, span_y = inside ? far : 0.0f;
  const float step = (span_y - span_x) / (float)kMarchSteps;
  const bool marching = span_x <= span_y;  // uniform: the same kernel arguments in every thread

  uint32_t first = kNoCrossing;
  if (marching) {
    gaps[tid] = gap_at(a, d, tid == 0u ? span_x : span_x + step * (float)tid);
    gaps[tid + 256u] = gap_at(a, d, span_x + step * (float)(tid + 256u));
    if (tid == 0u) gaps[kMarchSteps] = gap_at(a, d, span_x + step * (float)kMarchSteps);
    __syncthreads();
    // crossing i: gap_i <= 0 && gap_(i-1) > 0, for i = tid + 1 and i = tid + 257
    const bool c1 = gaps[tid + 1u] <= 0.0f && gaps[tid] > 0.0f;
    const bool c2 = gaps[tid + 257u] <= 0.0f && gaps[tid + 256u] > 0.0f;
    const unsigned long long b1 = __ballot(c1), b2 = __ballot(c2);
    uint32_t mine = kNoCrossing;
    if (b1) {
      mine = wave * 64u + (uint32_t)__builtin_ctzll(b1) + 1u;
    } else if (b2) {
      mine = 256u + wave * 64u + (uint32_t)__builtin_ctzll(b2) + 1u;
    }
    if (lane == 0u) wave_first[wave] = mine;
    __syncthreads();
    first = min(min(wave_first[0], wave_first[1]), min(wave_first[2], wave_first[3]));
  }
  if (wave != 0u) return;

  float wx = 0.0f, wy = 0.0f, wz = 0.0f;
  uint32_t valid = 0u, origin[4] = {0u, 0u, 0u, 0u};
  if (first != kNoCrossing) {
    // B5; first is in 1 .. 512
    float lo = first == 1u ? span_x : span_x + step * (float)(first - 1u), hi = span_x + step * (float)first;
#pragma unroll 1
    for (uint32_t j = 0; j < kRefineSteps; j++) {
      const float mid = (lo + hi) * 0.5f;
      if (gap_at(a, d, mid) > 0.0f) {
        lo = mid;
      } else {
        hi = mid;
      }
    }
    wx = B.ray_origin[0] + d.x * hi, wy = B.ray_origin[1] + d.y * hi, wz = B.ray_origin[2] + d.z * hi;
    valid = 1u;
    // B6
    const float radius = B.radius_texels + 1.0f;
    const float fw = (float)B.resolution[0], fh = (float)B.resolution[1];
    const float cx = ((wx - B.world_min[0]) * B.inv_world_size[0]) * fw, cy = ((wz - B.world_min[1]) * B.inv_world_size[1]) * fh;
    const float sx = (float)B.patch_count[0] / fw, sy = (float)B.patch_count[1] / fh;
    origin[0] = cvt_u32_sat(fmaxf(floorf(cx - radius), 0.0f));
    origin[1] = cvt_u32_sat(fmaxf(floorf(cy - radius), 0.0f));
    origin[2] = cvt_u32_sat(fmaxf(floorf((cx - radius) * sx), 0.0f));
    origin[3] = cvt_u32_sat(fmaxf(floorf((cy - radius) * sy), 0.0f));
  }
  if (lane == 0u) {
    a.hit[0] = asu(wx), a.hit[1] = asu(wy), a.hit[2] = asu(wz), a.hit[3] = valid;
    a.region[0] = origin[0], a.region[1] = origin[1], a.region[2] = origin[2], a.region[3] = origin[3];
  }
}

// B7 - B10
__global__ __launch_bounds__(256) void k_terrain_brush_apply(TerrainBrushArgs a) {
  const oxc_terrain_brush_params& B = a.p;
  const uint2 hit_xy = reinterpret_cast<const uint2*>(a.hit)[0], hit_zw = reinterpret_cast<const uint2*>(a.hit)[1];  // one address for the whole wave; 8-byte aligned
  const uint4 hit = make_uint4(hit_xy.x, hit_xy.y, hit_zw.x, hit_zw.y);
  if (hit.w == 0u) return;
  const uint2 t = tile_pixel();
  const uint32_t w = B.resolution[0], h = B.resolution[1];
  const float cx = ((asf(hit.x) - B.world_min[0]) * B.inv_world_size[0]) * (float)w, cy = ((asf(hit.z) - B.world_min[1]) * B.inv_world_size[1]) * (float)h;
  const long long radius = (long long)cvt_i32_sat(ceilf(B.radius_texels));
  const long long sx = ((long long)cvt_i32_sat(floorf(cx)) - radius) + (long long)t.x, sy = ((long long)cvt_i32_sat(floorf(cy)) - radius) + (long long)t.y;
  if (sx < 0 || sy < 0 || sx >= (long long)w || sy >= (long long)h) return;
  const int x = (int)sx, y = (int)sy;

  // B8
  if (B.radius_texels <= 0.0f) return;
  const float dx = ((float)x + 0.5f) - cx, dy = ((float)y + 0.5f) - cy;
  const float distance = __builtin_sqrtf(dx * dx + dy * dy);
  const float s = saturate_f(1.0f - distance / B.radius_texels);
  const float smoothed = ((s * s) * s) * (s * (s * 6.0f - 15.0f) + 10.0f);
  const float falloff = pow_rule(smoothed, fmaxf(B.falloff, 1e-3f));
  if (falloff <= 0.0f) return;
  const float amount = falloff * B.strength;
  const size_t at = (size_t)y * w + (size_t)x;

  if (B.mode == OXC_TERRAIN_BRUSH_PAINT_LAYER) {
    // B9
    const float k = saturate_f(amount);
    const uint32_t pw = a.splat_edit[at];
    const float p0 = (float)(pw & 0xFFu) / 255.0f, p1 = (float)((pw >> 8) & 0xFFu) / 255.0f, p2 = (float)((pw >> 16) & 0xFFu) / 255.0f, p3 = (float)(pw >> 24) / 255.0f;
    const float t0 = B.layer == 1u ? 1.0f : 0.0f, t1 = B.layer == 2u ? 1.0f : 0.0f, t2 = B.layer == 3u ? 1.0f : 0.0f;
    a.splat_edit[at] = pack_unorm(lerp_f(p0, t0, k)) | (pack_unorm(lerp_f(p1, t1, k)) << 8) | (pack_unorm(lerp_f(p2, t2, k)) << 16) | (pack_unorm(lerp_f(p3, 1.0f, k)) << 24);
    return;
  }

  // B10
  const float height = load_height(a, x, y);
  float delta = amount;  // Raise
  if (B.mode == OXC_TERRAIN_BRUSH_SMOOTH) {
    float sum = 0.0f;
#pragma unroll
    for (int oy = -2; oy <= 2; oy++) {
#pragma unroll
      for (int ox = -2; ox <= 2; ox++) sum = sum + load_height(a, x + ox, y + oy);
    }
    delta = (sum / 25.0f - height) * amount;
  } else if (B.mode == OXC_TERRAIN_BRUSH_FLATTEN) {
    delta = (B.flatten_height - height) * amount;
  } else if (B.mode == OXC_TERRAIN_BRUSH_NOISE) {
    delta = noised((float)x * 0.05f, (float)y * 0.05f, 0.0f, 0.0f).x * amount;
  }
  a.height_edit[at] = clamp_lo_hi(a.height_edit[at] + delta, -1.0f, 1.0f);
}
}  // namespace

void launch_terrain_brush_trace(const TerrainBrushArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_terrain_brush_trace, dim3(1), dim3(256), 0, s, a); }

void launch_terrain_brush_apply(const TerrainBrushArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_terrain_brush_apply, dim3(a.groups, a.groups), dim3(256), 0, s, a); }

}  // namespace oxc
