// oxcull_vsm_resolve.hip -- VSM shadow resolve (gfx950): the resolve_shadowmaps pass of Oxylus/src/Render/Passes/Shadowmaps.cpp:756-822
// (passes/resolve_shadowmaps.slang) as one compute launch.  Rules: include/oxcull.h, oxc_resolve_shadowmap; design and measurements:
// DESIGN.md section 12.
//
//   k_vsm_resolve_shadow   one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block): the taps of neighbouring pixels
//                          land in the same few pages, so a wave's page-table words and physical texels share cache lines.  Everything
//                          that is uniform per call -- the inverse view-projection, the clipmap thresholds, the light's tangent basis,
//                          the texel length, the 16 + 24 Hammersley points -- is worked out once on the host by the stated binary32 rules
//                          and travels in the kernel arguments (scalar loads); the clipmap records sit in LDS.  A pixel with depth 0
//                          stores 1.0 and leaves; a wave whose 64 pixels are all sky is gone after one load and one store.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and square
// root are the IEEE ones, the rotation pair is evaluated in binary64.
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr uint32_t kBacked = 4u;
constexpr float kMiss = -1.0f;  // VSM_DEPTH_MISS

OXC_DEV float row(const float* c, int r, const V3& p) { return ((OXC_M(c, r, 0) * p.x + OXC_M(c, r, 1) * p.y) + OXC_M(c, r, 2) * p.z) + OXC_M(c, r, 3); }

// pcg2d on (x, y), u32 wrap-around
OXC_DEV void pcg2d(uint32_t& x, uint32_t& y) {
  x = x * 1664525u + 1013904223u;
  y = y * 1664525u + 1013904223u;
  x += y * 1664525u;
  y += x * 1664525u;
  x ^= x >> 16;
  y ^= y >> 16;
  x += y * 1664525u;
  y += x * 1664525u;
  x ^= x >> 16;
  y ^= y >> 16;
}

// sample_vsm_shadow_depth: the depth clipmap `ci` holds for world position p, or kMiss
OXC_DEV float tap(const VsmResolveArgs& a, const float* cms, int ci, const V3& p) {
  if (ci < 0 || ci >= (int)a.layers) return kMiss;
  const float* c = cms + ci * 19;
  const float hx = row(c, 0, p), hy = row(c, 1, p), hw = row(c, 3, p);
  const float su = (hx / hw + 1.0f) * 0.5f, sv = (hy / hw + 1.0f) * 0.5f;
  if (!(su >= 0.0f && su <= 1.0f && sv >= 0.0f && sv <= 1.0f)) return kMiss;  // outside, or NaN
  uint32_t wx, wy;
  if (!wrapped_page(c, su, sv, a.fn, (int)a.n, wx, wy)) return kMiss;
  const uint32_t e = a.page_table[((uint32_t)ci * a.n + wy) * a.n + wx];
  if (!(e & kBacked)) return kMiss;
  const uint32_t addr = e >> 16;
  if (addr >= a.phys_count) return kMiss;  // names no physical page: never loaded
  const uint32_t tx = (uint32_t)(int)floorf(su * a.fV) % a.page_size, ty = (uint32_t)(int)floorf(sv * a.fV) % a.page_size;
  const uint32_t X = (addr % a.phys_side) * a.page_size + tx, Y = (addr / a.phys_side) * a.page_size + ty;
  return a.physical[(size_t)Y * a.physical_size + X];
}

template <bool STATS>
OXC_DEV float tap_with_fallback(const VsmResolveArgs& a, const float* cms, int base, const V3& p, uint32_t* st) {
  float d = tap(a, cms, base, p);
  if (STATS) st[1]++;
  if (d != kMiss) return d;
  d = tap(a, cms, base - 1, p);
  if (d != kMiss) {
    if (STATS) st[3]++;
    return d;
  }
  d = tap(a, cms, base + 1, p);
  if (STATS) st[d != kMiss ? 4 : 2]++;
  return d;
}
}  // namespace

template <bool STATS>
__global__ __launch_bounds__(256) void k_vsm_resolve_shadow(VsmResolveArgs a) {
  __shared__ float cms[16 * 19];
  for (uint32_t i = threadIdx.x; i < a.layers * 19; i += blockDim.x) cms[i] = a.clipmaps[i];
  __syncthreads();
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const size_t pix = (size_t)py * a.w + px;
  const float d = a.depth[pix];
  if (d == 0.0f) {  // sky (a NaN depth is not)
    a.out[pix] = 1.0f;
    return;
  }
  uint32_t st[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // STATS: {non-sky pixels, taps, taps no clipmap served, served by base - 1, by base + 1, hard, no blocker, all blockers}

  // pixel set-up
  const float u = ((float)px + 0.5f) / (float)a.w, v = ((float)py + 0.5f) / (float)a.h;
  V3 world;
  const int base = pixel_world_and_clipmap(a, u, v, d, world);

  // flat_N = normalize(oct_to_vec3(normal.ba))
  const V3 N = normalize3(normalize3(oct_normal_ba(a.normal[pix * 2u + 1u])));

  uint32_t hx = px, hy = py;
  pcg2d(hx, hy);
  const float nx = (float)(hx >> 8) * 0x1p-24f, ny = (float)(hy >> 8) * 0x1p-24f;

  // pcss_shadow
  const V3 L = {a.light[0], a.light[1], a.light[2]}, T = {a.tangent[0], a.tangent[1], a.tangent[2]}, B = {a.bitangent[0], a.bitangent[1], a.bitangent[2]};
  const float NoL = fmaxf(dot3(N.x, N.y, N.z, L.x, L.y, L.z), 0.0f);  // a NaN becomes 0
  const float cts = asf((uint32_t)(127 + base + 1) << 23) * a.texel_len;  // pow(2.0, f32(base + 1)), exact
  const float b = (1.41421356f * cts) * 0.5f;
  const V3 NxL = {N.y * L.z - N.z * L.y, N.z * L.x - N.x * L.z, N.x * L.y - N.y * L.x};
  const float slope = (b * len3(NxL.x, NxL.y, NxL.z)) / fmaxf(NoL, 0.1f);
  const float base_bias = (0x1p-22f + b) + (NoL < 0.99f ? slope : b);
  const float now = cts * (1.0f + 2.0f * (1.0f - NoL));
  const V3 owp = {world.x + N.x * now, world.y + N.y * now, world.z + N.z * now};
  const float* cb = cms + base * 19;
  const float d_recv = row(cb, 2, owp) / row(cb, 3, owp);
  const float d_recv_world = d_recv * a.z_length;
  const float center = tap_with_fallback<STATS>(a, cms, base, owp, st);

  float accum = 0.0f;
  uint32_t blockers = 0, valid = 0;
#pragma unroll 1
  for (uint32_t i = 0; i < 16u; i++) {
    const float t0 = a.ham[i][0] + nx, t1 = a.ham[i][1] + ny;
    const float xi0 = t0 - floorf(t0), xi1 = t1 - floorf(t1);
    const float rad = __builtin_sqrtf(xi0) * 0.1f;
    float cs, sn;
    cos_sin_turn(xi1, cs, sn);
    const V3 p = {owp.x + rad * (T.x * cs + B.x * sn), owp.y + rad * (T.y * cs + B.y * sn), owp.z + rad * (T.z * cs + B.z * sn)};
    const float pcf_bias = 2.0f * rad;
    const float bias_norm = a.inv_z_length * (base_bias + (pcf_bias + (0.0f - pcf_bias) * NoL));
    const float depth = tap_with_fallback<STATS>(a, cms, base, p, st);
    if (depth == kMiss) continue;
    valid++;
    if (depth + bias_norm < d_recv) {
      accum += depth * a.z_length;
      blockers++;
    }
  }
  const float hard = center == kMiss ? 1.0f : (center + a.inv_z_length * base_bias < d_recv ? 0.0f : 1.0f);
  float result;
  if (valid == 0u) {
    result = hard;
    if (STATS) st[5]++;
  } else if (blockers == 0u) {
    result = 1.0f;
    if (STATS) st[6]++;
  } else if (blockers == valid) {
    result = 0.0f;
    if (STATS) st[7]++;
  } else {
    const float d_blocker_world = accum / (float)blockers;
    const float pcf_radius = fminf(0.1f, (d_recv_world - d_blocker_world) * 0.002f);
    float vis = 0.0f;
    uint32_t vpcf = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < 24u; i++) {
      const float t0 = a.ham[16u + i][0] + ny, t1 = a.ham[16u + i][1] + nx;  // noise.yx
      const float xi0 = t0 - floorf(t0), xi1 = t1 - floorf(t1);
      const float rad = __builtin_sqrtf(xi0) * pcf_radius;
      float cs, sn;
      cos_sin_turn(xi1, cs, sn);
      const V3 p = {owp.x + rad * (T.x * cs + B.x * sn), owp.y + rad * (T.y * cs + B.y * sn), owp.z + rad * (T.z * cs + B.z * sn)};
      const float pcf_bias = 2.0f * rad;
      const float bias_norm = a.inv_z_length * (base_bias + (pcf_bias + (0.0f - pcf_bias) * NoL));
      const float depth = tap_with_fallback<STATS>(a, cms, base, p, st);
      if (depth == kMiss) continue;
      vpcf++;
      if (depth + bias_norm >= d_recv) vis += 1.0f;
    }
    if (vpcf == 0u) {
      result = hard;
      if (STATS) st[5]++;
    } else {
      result = vis / (float)vpcf;
    }
  }
  a.out[pix] = result;
  if (STATS) {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (st[k]) atomicAdd(&a.stats[k], st[k]);
  }
}

void launch_vsm_resolve(const VsmResolveArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  if (a.stats)
    hipLaunchKernelGGL(k_vsm_resolve_shadow<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_vsm_resolve_shadow<false>, grid, dim3(256), 0, s, a);
}

}  // namespace oxc
