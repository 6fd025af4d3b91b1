// oxcull_visbuffer_device.hpp -- what the draws into the depth|vis image share beyond the rasteriser rules of oxcull_raster_device.hpp: the
// set-up triangle record of the big list, its per-triangle preparation, the (0, 1] depth test with the 64-bit atomicMax, the in-wave
// record, and the hand-over of a set-up triangle to the segmented big list (or, when that is full, its walk by the producing lane).
// oxc_draw_visbuffer (oxcull_raster.hip) and oxc_draw_terrain (oxcull_terrain_draw.hip) include it; k_draw_big and k_draw_big_tiles of
// oxcull_raster.hip consume the big list of either.  Compiled without contraction by the including files.
#pragma once

#include "oxcull_raster_device.hpp"

namespace oxc {

struct TriSetup {
  int32_t x[3], y[3];  // 24.8 fixed point, oriented with positive area
  float z[3];
  uint32_t vis;
};
constexpr int64_t kBigTile = 64;

static_assert(sizeof(TriSetup) == kTriSetupBytes, "layout");

struct TriRaster {
  int64_t X[3], Y[3];
  float z[3];
  uint32_t vis;
  int64_t area, b0, b1, b2;
  int64_t px0, px1, py0, py1;
  double inv_area;
  int64_t dx0, dx1, dx2, dy0, dy1, dy2;  // change of the three edge functions per pixel step in x / in y (exact)
};

OXC_DEV void tri_prepare(const TriSetup& t, uint32_t W, uint32_t H, TriRaster& r) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r.X[k] = t.x[k];
    r.Y[k] = t.y[k];
    r.z[k] = t.z[k];
  }
  r.vis = t.vis;
  r.area = edge_fn(r.X[0], r.Y[0], r.X[1], r.Y[1], r.X[2], r.Y[2]);
  int32_t px0, py0, px1, py1;
  (void)pixel_box(t, (int32_t)W, (int32_t)H, px0, py0, px1, py1);
  r.px0 = px0, r.py0 = py0, r.px1 = px1, r.py1 = py1;
  r.b0 = edge_inclusive(r.X[1], r.Y[1], r.X[2], r.Y[2]) ? 0 : -1;
  r.b1 = edge_inclusive(r.X[2], r.Y[2], r.X[0], r.Y[0]) ? 0 : -1;
  r.b2 = edge_inclusive(r.X[0], r.Y[0], r.X[1], r.Y[1]) ? 0 : -1;
  r.inv_area = 1.0 / (double)r.area;  // one reciprocal per triangle
  // E(a->b)(p) = (bx - ax)(py - ay) - (by - ay)(px - ax): one pixel = 256 units
  r.dx0 = -(r.Y[2] - r.Y[1]) * 256;
  r.dy0 = (r.X[2] - r.X[1]) * 256;
  r.dx1 = -(r.Y[0] - r.Y[2]) * 256;
  r.dy1 = (r.X[0] - r.X[2]) * 256;
  r.dx2 = -(r.Y[1] - r.Y[0]) * 256;
  r.dy2 = (r.X[1] - r.X[0]) * 256;
}

// edge values (weights of corners 0, 1, 2) at the centre of pixel (px, py)
OXC_DEV void tri_edges(const TriRaster& r, int64_t px, int64_t py, int64_t& e0, int64_t& e1, int64_t& e2) {
  const int64_t cx = px * 256 + 128, cy = py * 256 + 128;
  e0 = edge_fn(r.X[1], r.Y[1], r.X[2], r.Y[2], cx, cy);
  e1 = edge_fn(r.X[2], r.Y[2], r.X[0], r.Y[0], cx, cy);
  e2 = edge_fn(r.X[0], r.Y[0], r.X[1], r.Y[1], cx, cy);
}
// fs of a covered pixel: depth test, then the maximum of depth|vis (I: the width of the edge values, P: of the pixel coordinates).
// tally, here and in the walkers below: the calling lane's count of fragments that passed the depth range, for a counting instantiation
// (oxc_draw_terrain's); the default null folds away, and the kernels that pass none compile to what they were.
template <class I, class P>
OXC_DEV void fragment(I e0, I e1, I e2, float z0, float z1, float z2, double inv_area, uint32_t vis, P px, P py, uint32_t W, unsigned long long* visdepth,
                      uint32_t* tally = nullptr) {
  const float zf = interpolate_depth(e0, e1, e2, z0, z1, z2, inv_area);
  if (!(zf > 0.0f) || zf > 1.0f) return;
  if (tally) ++*tally;
  const unsigned long long packed = ((unsigned long long)asu(zf) << 32) | vis;
  // (reading the stored value first to skip occluded fragments was measured slower: 1.61 -> 2.15 ms per frame)
  atomicMax(&visdepth[(size_t)py * W + (size_t)px], packed);
}
OXC_DEV void tri_fragment(const TriRaster& r, int64_t e0, int64_t e1, int64_t e2, int64_t px, int64_t py, uint32_t W, unsigned long long* visdepth,
                          uint32_t* tally = nullptr) {
  if (covered(e0, e1, e2, r.b0, r.b1, r.b2)) fragment(e0, e1, e2, r.z[0], r.z[1], r.z[2], r.inv_area, r.vis, px, py, W, visdepth, tally);
}

// SmallTri with the triangle's vis value (56 bytes).  A record of its own, not SmallTri plus a trailing word: with vis behind misc
// k_draw_setup moves its record with two more LDS instructions, and the draw at 3840 x 2160 measured 0.06 ms (0.6 %) over the parent,
// twice the parent's own spread in that session (profiles/raster_device_timing.jsonl).
struct TriLds {
  int32_t x[3], y[3];
  float z[3];
  uint32_t vis;
  uint32_t inv_area_lo, inv_area_hi;
  uint32_t box, misc;
};

// setup_tri with cullMode eBack for the draw's extent
OXC_DEV bool tri_finish(const DrawArgs& a, const float* c0, const float* c1, const float* c2, uint32_t vis, TriSetup& out, int32_t& spread) {
  out.vis = vis;
  return setup_tri<true>((float)a.width, (float)a.height, c0, c1, c2, out, spread);
}

// one lane walks a pixel rectangle of its triangle
OXC_DEV void walk_box(const DrawArgs& a, const TriRaster& r, int64_t x0, int64_t y0, int64_t x1, int64_t y1, uint32_t* tally = nullptr) {
  int64_t r0, r1, r2;  // edge values at the start of the row: stepped exactly (integers) instead of re-multiplied
  tri_edges(r, x0, y0, r0, r1, r2);
  for (int64_t py = y0; py <= y1; py++) {
    int64_t e0 = r0, e1 = r1, e2 = r2;
    for (int64_t px = x0; px <= x1; px++) {
      tri_fragment(r, e0, e1, e2, px, py, a.width, a.visdepth, tally);
      e0 += r.dx0;
      e1 += r.dx1;
      e2 += r.dx2;
    }
    r0 += r.dy0;
    r1 += r.dy1;
    r2 += r.dy2;
  }
}

// A triangle whose pixel box exceeds kSmallSpan goes to segment `seg` of the big list (k_draw_big: one wave per triangle).  A triangle
// that does not fit its segment any more is walked by this lane (slow, correct).
OXC_DEV void push_big(const DrawArgs& a, const TriSetup& t, uint32_t seg, uint32_t* tally = nullptr) {
  const uint32_t slot = atomicAdd(a.big_seg_counts + seg * kBigSegStride, 1u);
  if (slot < a.big_seg_capacity) {
    a.big_list[(size_t)seg * a.big_seg_capacity + slot] = t;
    return;
  }
  TriRaster r;
  tri_prepare(t, a.width, a.height, r);
  for (int64_t py = r.py0; py <= r.py1; py++)
    for (int64_t px = r.px0; px <= r.px1; px++) {
      int64_t e0, e1, e2;
      tri_edges(r, px, py, e0, e1, e2);
      tri_fragment(r, e0, e1, e2, px, py, a.width, a.visdepth, tally);
    }
}

// rasterise one set-up triangle from this lane (small ones) or queue it for k_draw_big
OXC_DEV void tri_emit(const DrawArgs& a, const TriSetup& t, uint32_t seg, uint32_t* tally = nullptr) {
  TriRaster r;
  tri_prepare(t, a.width, a.height, r);
  if (r.px1 < r.px0 || r.py1 < r.py0) return;
  const bool small = (r.px1 - r.px0) < kSmallSpan && (r.py1 - r.py0) < kSmallSpan;
  if (!small) {
    push_big(a, t, seg, tally);
    return;
  }
  walk_box(a, r, r.px0, r.py0, r.px1, r.py1, tally);
}

}  // namespace oxc
