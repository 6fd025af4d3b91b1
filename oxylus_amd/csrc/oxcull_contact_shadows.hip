// oxcull_contact_shadows.hip -- contact shadows (gfx950): the contact_shadows pass of Oxylus/src/Render/RendererInstance.cpp:990-1020
// (passes/contact_shadows.slang + raymarch.slang) as one compute launch.  Rules: include/oxcull.h, oxc_contact_shadows; design and
// measurements: DESIGN.md section 13.
//
//   k_contact_shadows   one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block): the ray of a pixel is a few pixels
//                       long, so the taps of a wave fall into the depth rows its own pixels were loaded from.  Everything that is uniform
//                       per call -- the three matrices, normalize(sun_dir) * shadow_length, depth_thickness, 1.0f + bias, the extents --
//                       is worked out once on the host by the stated binary32 rules and travels in the kernel arguments (scalar loads).
//                       A pixel with depth 0 stores 1.0 and leaves; a wave whose 64 pixels are all sky is gone after one load and one
//                       store.  The five texels of a tap are loaded unconditionally at clamped coordinates, in one batch.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and square
// root are the IEEE ones.
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
// mul(M, (x, y, z, w)).r
OXC_DEV float row4(const float* m, int r, float x, float y, float z, float w) {
  return ((OXC_M(m, r, 0) * x + OXC_M(m, r, 1) * y) + OXC_M(m, r, 2) * z) + OXC_M(m, r, 3) * w;
}
}  // namespace

template <bool STATS>
__global__ __launch_bounds__(256) void k_contact_shadows(ContactShadowsArgs a) {
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const size_t pix = (size_t)py * a.w + px;
  const float d = a.depth[pix];
  if (d == 0.0f) {  // sky (a NaN depth is not)
    a.out[pix] = 1.0f;
    return;
  }
  const int wm1 = (int)a.w - 1, hm1 = (int)a.h - 1;

  // set-up: the pixel in clip space, its world position, the ray's end in world space
  const float csx = (((float)px + 0.5f) / a.fw) * 2.0f - 1.0f, csy = (((float)py + 0.5f) / a.fh) * 2.0f - 1.0f, csz = d;
  const float hw = row1(a.inv_pv, 3, csx, csy, csz);
  const float wx = row1(a.inv_pv, 0, csx, csy, csz) / hw + a.ray[0];
  const float wy = row1(a.inv_pv, 1, csx, csy, csz) / hw + a.ray[1];
  const float wz = row1(a.inv_pv, 2, csx, csy, csz) / hw + a.ray[2];

  // the ray's end in clip space
  const float vx = row1(a.view, 0, wx, wy, wz), vy = row1(a.view, 1, wx, wy, wz), vz = row1(a.view, 2, wx, wy, wz), vw = row1(a.view, 3, wx, wy, wz);
  const float pw = row4(a.proj, 3, vx, vy, vz, vw);
  const float ex = row4(a.proj, 0, vx, vy, vz, vw) / pw, ey = row4(a.proj, 1, vx, vy, vz, vw) / pw, ez = row4(a.proj, 2, vx, vy, vz, vw) / pw;
  const float sg = sign_f(ez);
  const float endx = csx + (ex - csx) * sg, endy = csy + (ey - csy) * sg, endz = csz + (ez - csz) * sg;
  // start clip
  float dx = endx - csx, dy = endy - csy, dz = endz - csz;
  const float m = fmaxf(((dx < 0.0f ? 1.0f : -1.0f) - csx) / dx, ((dy < 0.0f ? 1.0f : -1.0f) - csy) / dy);
  const float mv = fmaxf(0.0f, m);
  const float sx = csx + dx * mv, sy = csy + dy * mv, sz = csz + dz * mv;
  // end clip
  dx = endx - sx, dy = endy - sy, dz = endz - sz;
  const float qx = ((dx >= 0.0f ? 1.0f : -1.0f) - sx) / dx, qy = ((dy >= 0.0f ? 1.0f : -1.0f) - sy) / dy, qz = ((dz >= 0.0f ? 1.0f : 0.0f) - sz) / dz;
  const float qmin = fminf(fminf(qx, qy), qz);
  const float clip = fminf(1.0f, qmin);
  const float rex = sx + dx * clip, rey = sy + dy * clip, rez = sz + dz * clip;

  // step count
  const float lx = ((rex * 0.5f + 0.5f) - (sx * 0.5f + 0.5f)) * a.fw, ly = ((rey * 0.5f + 0.5f) - (sy * 0.5f + 0.5f)) * a.fh;
  const uint32_t len_u = cvt_u32_sat(floorf(__builtin_sqrtf(lx * lx + ly * ly)));
  const uint32_t n = max(2u, min(a.steps, len_u));
  const float fn = (float)n;
  const float dirx = rex - sx, diry = rey - sy, dirz = rez - sz;

  // linear march
  bool intersected = false;
  float distance = 0.0f, penetration = 0.0f;
  uint32_t taps = 0;
#pragma unroll 1
  for (uint32_t step = 0; step < n; step++) {
    const float t = ((float)step + 1.0f) / fn;
    const float cx = sx + dirx * t, cy = sy + diry * t, cz = sz + dirz * t;
    const float ux = (cx * 0.5f + 0.5f) * a.fw, uy = (cy * 0.5f + 0.5f) * a.fh;
    const float ray_depth = 1.0f / cz;
    const float gx = ux - 0.5f, gy = uy - 0.5f;
    const float ix = floorf(gx), iy = floorf(gy);
    const float fx = gx - ix, fy = gy - iy;
    const int bx = clamp_i(cvt_i32_sat(ix), -1, wm1), by = clamp_i(cvt_i32_sat(iy), -1, hm1);  // i + 1 cannot wrap after this
    const int x0 = max(bx, 0), x1 = min(bx + 1, wm1), y0 = max(by, 0), y1 = min(by + 1, hm1);
    const int nx = clamp_i(cvt_i32_sat(floorf(ux)), 0, wm1), ny = clamp_i(cvt_i32_sat(floorf(uy)), 0, hm1);
    const float* r0 = a.depth + (size_t)y0 * a.w;
    const float* r1 = a.depth + (size_t)y1 * a.w;
    const float t00 = r0[x0], t10 = r0[x1], t01 = r1[x0], t11 = r1[x1], tn = a.depth[(size_t)ny * a.w + nx];
    const float top = t00 + (t10 - t00) * fx, bot = t01 + (t11 - t01) * fx;
    const float linear_depth = 1.0f / (top + (bot - top) * fy), unfiltered_depth = 1.0f / tn;
    distance = fmaxf(linear_depth, unfiltered_depth) * a.one_plus_bias - ray_depth;
    penetration = ray_depth - fminf(linear_depth, unfiltered_depth);
    taps++;
    if (distance < 0.0f) {
      intersected = true;
      break;
    }
  }

  float result = 1.0f;
  const bool hit = intersected && penetration < a.depth_thickness && distance < a.depth_thickness;
  if (hit) {
    const float frac = penetration / a.depth_thickness;
    const float s = fminf(fmaxf((frac - 1.0f) / a.edge_span, 0.0f), 1.0f);
    result = 1.0f - (s * s) * (3.0f - 2.0f * s);
  }
  a.out[pix] = result;
  if (STATS) {
    // {non-sky, taps, miss, hit 0.0, hit inside (0, 1), hit 1.0, rejected, n lower clamp, n between, n upper clamp, end clip, start moved}
    const uint32_t lim = min(a.steps, len_u);
    const uint32_t outcome = !intersected ? 2u : !hit ? 6u : result == 0.0f ? 3u : result == 1.0f ? 5u : 4u;
    const uint32_t ncls = lim < 2u ? 7u : len_u >= a.steps ? 9u : 8u;
    atomicAdd(&a.stats[0], 1u);
    atomicAdd(&a.stats[1], taps);
    atomicAdd(&a.stats[outcome], 1u);
    atomicAdd(&a.stats[ncls], 1u);
    if (clip < 1.0f) atomicAdd(&a.stats[10], 1u);
    if (mv > 0.0f) atomicAdd(&a.stats[11], 1u);
  }
}

void launch_contact_shadows(const ContactShadowsArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  if (a.stats)
    hipLaunchKernelGGL(k_contact_shadows<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_contact_shadows<false>, grid, dim3(256), 0, s, a);
}

}  // namespace oxc
