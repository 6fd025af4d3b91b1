// oxcull_pixel_device.hpp -- the device rules the VSM page update and the per-pixel passes (shadow resolve, contact shadows, ambient
// occlusion) share: one copy each, so that two kernels which must agree on a pixel's clipmap, page or normal cannot drift apart.
// Every float operation keeps the order and rounding include/oxcull.h states; the including files are compiled without contraction.
#pragma once

#include "oxcull_device.hpp"

namespace oxc {

struct V3 {
  float x, y, z;
};

OXC_DEV V3 normalize3(const V3& v) {
  const float l = len3(v.x, v.y, v.z);
  return {v.x / l, v.y / l, v.z / l};
}

OXC_DEV int floor_mod_i(int x, int n) {
  const int r = x % n;
  return r < 0 ? r + n : r;
}
OXC_DEV float saturate_f(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }  // a NaN becomes 0 (max(NaN, 0) = 0)
OXC_DEV float sign_f(float a) { return a > 0.0f ? 1.0f : a < 0.0f ? -1.0f : 0.0f; }
OXC_DEV int clamp_i(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The pixel of this thread: an 8 x 8 pixel tile per wave, a 16 x 16 tile per block of 256 threads.
OXC_DEV uint2 tile_pixel() {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  return make_uint2(blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u), blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3));
}

// mul(m, (u * 2 - 1, v * 2 - 1, d, 1)).xyz / .w
OXC_DEV void unproject(const float* m, float u, float v, float d, float& x, float& y, float& z) {
  const float nx = u * 2.0f - 1.0f, ny = v * 2.0f - 1.0f;
  const float hx = ((OXC_M(m, 0, 0) * nx + OXC_M(m, 0, 1) * ny) + OXC_M(m, 0, 2) * d) + OXC_M(m, 0, 3);
  const float hy = ((OXC_M(m, 1, 0) * nx + OXC_M(m, 1, 1) * ny) + OXC_M(m, 1, 2) * d) + OXC_M(m, 1, 3);
  const float hz = ((OXC_M(m, 2, 0) * nx + OXC_M(m, 2, 1) * ny) + OXC_M(m, 2, 2) * d) + OXC_M(m, 2, 3);
  const float hw = ((OXC_M(m, 3, 0) * nx + OXC_M(m, 3, 1) * ny) + OXC_M(m, 3, 2) * d) + OXC_M(m, 3, 3);
  x = hx / hw;
  y = hy / hw;
  z = hz / hw;
}

// The wrapped page coordinate of clipmap uv (su, sv) in [0, 1]^2, `c` the clipmap's record (its page offsets in c[16], c[17]), fn = (float)n;
// false for uv == 1.0, which lands on virt == n.
OXC_DEV bool wrapped_page(const float* c, float su, float sv, float fn, int n, uint32_t& wx, uint32_t& wy) {
  const int vx = (int)floorf(su * fn), vy = (int)floorf(sv * fn);
  if (vx > n - 1 || vy > n - 1) return false;
  const int ox = __builtin_bit_cast(int, c[16]), oy = __builtin_bit_cast(int, c[17]);
  wx = (uint32_t)floor_mod_i(vx + floor_mod_i(ox, n), n);
  wy = (uint32_t)floor_mod_i(vy + floor_mod_i(oy, n), n);
  return true;
}

// oct_to_vec3(normal.ba) before any normalisation; `nba` = the texel's second word, .b in the low half, .a in the high half
OXC_DEV V3 oct_normal_ba(uint32_t nba) {
  const float ex = dequantize_half(nba & 0xFFFFu), ey = dequantize_half(nba >> 16);
  V3 o;
  o.z = (1.0f - __builtin_fabsf(ex)) - __builtin_fabsf(ey);
  const float sx = ex >= 0.0f ? 1.0f : -1.0f, sy = ey >= 0.0f ? 1.0f : -1.0f;
  const bool fold = o.z < 0.0f;
  o.x = fold ? (1.0f - __builtin_fabsf(ey)) * sx : ex;
  o.y = fold ? (1.0f - __builtin_fabsf(ex)) * sy : ey;
  return o;
}

// (cos, sin) of 2 pi t, t a binary32 in [0, 1): exact reduction to an octant, two binary64 polynomials by Horner, one rounding each
// (the rotation rule of oxc_resolve_shadowmap, step 6 of its header block; oxc_generate_ambient_occlusion turns its slices by it too).
OXC_DEV void cos_sin_turn(float t, float& cs, float& sn) {
  const float q4 = t * 4.0f;  // exact
  const float kf = floorf(q4);
  const float f = q4 - kf;  // exact, in [0, 1)
  const bool swap = f > 0.5f;
  const float g = swap ? 1.0f - f : f;  // exact, in [0, 0.5]
  const double a = (double)g * 0x1.921fb54442d18p+0;
  const double z = a * a;
  const double ps = ((0x1.71de3a556c734p-19 * z + -0x1.a01a01a01a01ap-13) * z + 0x1.1111111111111p-7) * z + -0x1.5555555555555p-3;
  const double s = a + (a * z) * ps;
  const double pc = (((-0x1.27e4fb7789f5cp-22 * z + 0x1.a01a01a01a01ap-16) * z + -0x1.6c16c16c16c17p-10) * z + 0x1.5555555555555p-5) * z + -0x1.0000000000000p-1;
  const double c = 1.0 + z * pc;
  const float sf = (float)s, cf = (float)c;
  const float sq = swap ? cf : sf, cq = swap ? sf : cf;
  const int k = (int)kf;
  cs = k == 0 ? cq : k == 1 ? -sq : k == 2 ? -cq : sq;
  sn = k == 0 ? sq : k == 1 ? cq : k == 2 ? -sq : -cq;
}

}  // namespace oxc
