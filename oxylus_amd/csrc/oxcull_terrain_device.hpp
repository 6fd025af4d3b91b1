// oxcull_terrain_device.hpp -- the device rules the terrain maps (oxcull_terrain_maps.hip) and the terrain brush (oxcull_terrain_brush.hip)
// share: steps T2 and T3 of include/oxcull.h and the small helpers around them, one copy each.  Every float operation keeps the order and
// rounding the header states; the including files are compiled without contraction.
#pragma once

#include "oxcull_pixel_device.hpp"

namespace oxc {

constexpr float kK0 = 0.3183099f, kK1 = 0.3678794f;

struct V2 {
  float x, y;
};

OXC_DEV float clamp_lo_hi(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// Step B3's SampleLevel(LinearSamplerClamped, (u, v), 0) on a w x h terrain map before its loads: the clamped texel coordinates and
// weights per axis and the two row offsets.  The caller loads texel (x, y) at r{y} + ax.i{x} in its map's format and blends
// lerp(lerp(t00, t10, ax.f), lerp(t01, t11, ax.f), ay.f).
struct MapTaps {
  Axis ax, ay;
  size_t r0, r1;
};
OXC_DEV MapTaps map_taps(float u, float v, uint32_t w, uint32_t h) {
  const Axis ax = axis_at<false>(u, (float)w, (int)w - 1), ay = axis_at<false>(v, (float)h, (int)h - 1);
  return {ax, ay, (size_t)ay.i0 * w, (size_t)ay.i1 * w};
}

// T2; (sx, sy) = f32(seed) * (0.06711056f, 0.00583715f)
OXC_DEV V2 hash2(float x, float y, float sx, float sy) {
  const float qx = (x + sx) * kK0 + kK1, qy = (y + sy) * kK1 + kK0;
  const float t = fract_f((qx * qy) * (qx + qy));
  return {-1.0f + 2.0f * fract_f((16.0f * kK0) * t), -1.0f + 2.0f * fract_f((16.0f * kK1) * t)};
}

// T3: (value, derivative.x, derivative.y)
OXC_DEV V3 noised(float px, float py, float sx, float sy) {
  const float ix = floorf(px), iy = floorf(py);
  const float fx = px - ix, fy = py - iy;
  const float ux = ((fx * fx) * fx) * (fx * (fx * 6.0f - 15.0f) + 10.0f), uy = ((fy * fy) * fy) * (fy * (fy * 6.0f - 15.0f) + 10.0f);
  const float dux = ((30.0f * fx) * fx) * (fx * (fx - 2.0f) + 1.0f), duy = ((30.0f * fy) * fy) * (fy * (fy - 2.0f) + 1.0f);
  const V2 ga = hash2(ix, iy, sx, sy), gb = hash2(ix + 1.0f, iy, sx, sy), gc = hash2(ix, iy + 1.0f, sx, sy), gd = hash2(ix + 1.0f, iy + 1.0f, sx, sy);
  const float va = ga.x * fx + ga.y * fy;
  const float vb = gb.x * (fx - 1.0f) + gb.y * fy;
  const float vc = gc.x * fx + gc.y * (fy - 1.0f);
  const float vd = gd.x * (fx - 1.0f) + gd.y * (fy - 1.0f);
  const float k = ((va - vb) - vc) + vd;
  const float uxy = ux * uy;
  V3 r;
  r.x = ((va + ux * (vb - va)) + uy * (vc - va)) + uxy * k;
  r.y = (((ga.x + ux * (gb.x - ga.x)) + uy * (gc.x - ga.x)) + uxy * (((ga.x - gb.x) - gc.x) + gd.x)) + dux * ((uy * k + vb) - va);
  r.z = (((ga.y + ux * (gb.y - ga.y)) + uy * (gc.y - ga.y)) + uxy * (((ga.y - gb.y) - gc.y) + gd.y)) + duy * ((ux * k + vc) - va);
  return r;
}

}  // namespace oxc
