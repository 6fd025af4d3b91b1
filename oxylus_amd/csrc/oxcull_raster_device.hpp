// oxcull_raster_device.hpp -- the rasteriser rules the visbuffer draw (oxcull_raster.hip) and the VSM shadow draw (oxcull_vsm_draw.hip)
// share: one copy each, so that main-view depth and shadow depth of the same triangle cannot drift apart by a texel.  It owns the clip
// planes and the clipper, the index-entry decode and vertex fetch, the row builder, the 1/256 snap with its cull mode, the pixel box, the
// edge functions with the top-left rule and the depth interpolation, and the wave's small-box distribution pass.  The passes keep what
// differs between them: depth test, store, page logic, big lists and tiles, statistics, launches.
// Every float operation keeps the order and rounding include/oxcull.h states; the including files are compiled without contraction.
// Functions that read the argument struct are templates over it (DrawArgs, VsmDrawArgs): the fields they name are spelled alike in both.
#pragma once

#include "oxcull_device.hpp"
#include "oxcull_kernels.hpp"

namespace oxc {

constexpr int32_t kSmallSpan = 8;  // pixel box side of the in-wave path

// ---- clip rules ----------------------------------------------------------------------------------------------------------------------
// Clip planes of the stated rules (include/oxcull.h): w >= kClipWMin and the guard band |x|, |y| <= kClipGuard * w, which keeps every
// screen coordinate inside the +-2^20 px fixed-point range for extents up to 16384.
constexpr float kClipWMin = 0.0009765625f;  // 2^-10
constexpr float kClipGuard = 64.0f;
OXC_DEV float clip_distance(const float* v, int plane) {
  switch (plane) {
    case 0: return v[3] - kClipWMin;
    case 1: return kClipGuard * v[3] - v[0];
    case 2: return kClipGuard * v[3] + v[0];
    case 3: return kClipGuard * v[3] - v[1];
    default: return kClipGuard * v[3] + v[1];
  }
}

// 0: every corner inside every clip plane (the usual case); 1: crosses a plane (goes to the clipper); 2: all corners outside one plane
OXC_DEV int tri_clip_class(const float (&clip)[3][4]) {
  bool crosses = false;
#pragma unroll
  for (int pl = 0; pl < 5; pl++) {
    const bool i0 = clip_distance(clip[0], pl) >= 0.0f, i1 = clip_distance(clip[1], pl) >= 0.0f, i2 = clip_distance(clip[2], pl) >= 0.0f;
    if (!i0 && !i1 && !i2) return 2;
    crosses |= !(i0 && i1 && i2);
  }
  return crosses ? 1 : 0;
}

// Sutherland-Hodgman against the five planes.  In: the triangle's clip coordinates in poly[0][0..2].  Out: the corner count n (below 3:
// nothing left) and `cur`, the polygon being poly[cur][0..n-1]; the caller fans it from corner 0.  A new vertex on a crossing edge is always
// interpolated from its inside end I to its outside end O -- t = d(I) / (d(I) - d(O)), v = I + t (O - I), IEEE operations in that order --
// so the two triangles that share the edge get the same vertex whatever their winding.
OXC_DEV int clip_polygon(float (&poly)[2][9][4], int& cur) {
  int n = 3;
  cur = 0;
  for (int pl = 0; pl < 5 && n >= 3; pl++) {
    int m = 0;
    for (int k = 0; k < n; k++) {
      const float* p = poly[cur][k];
      const float* q = poly[cur][(k + 1) % n];
      const float dp = clip_distance(p, pl), dq = clip_distance(q, pl);
      const bool ip = dp >= 0.0f, iq = dq >= 0.0f;
      if (ip) {
        for (int c = 0; c < 4; c++) poly[cur ^ 1][m][c] = p[c];
        m++;
      }
      if (ip != iq) {
        const float* I = ip ? p : q;
        const float* O = ip ? q : p;
        const float dI = ip ? dp : dq, dO = ip ? dq : dp;
        const float t = dI / (dI - dO);
        for (int c = 0; c < 4; c++) poly[cur ^ 1][m][c] = I[c] + t * (O[c] - I[c]);
        m++;
      }
    }
    n = m;
    cur ^= 1;
  }
  return n;
}

// ---- index entries and the vertex fetch ----------------------------------------------------------------------------------------------
// An index-buffer entry: the packed u32 of visbuffer.slang:9-14 ((id << 8) | corner; << 9 with wide_triangle_index = 1) or, PAIR
// (wide_triangle_index = 2), the 8-byte pair {u32 meshlet_instance_index, u32 corner}.
template <bool PAIR>
struct IdxEntry {
  uint32_t d;
};
template <>
struct IdxEntry<true> {
  uint32_t id, corner;
};
template <bool PAIR, class Args>
OXC_DEV IdxEntry<PAIR> load_entry(const Args& a, size_t i) {
  if constexpr (PAIR) {
    const uint2 v = reinterpret_cast<const uint2*>(a.indices)[i];
    return IdxEntry<true>{v.x, v.y};
  } else {
    return IdxEntry<false>{a.indices[i]};
  }
}
template <bool PAIR, class Args>
OXC_DEV uint32_t entry_instance(const Args& a, const IdxEntry<PAIR>& e) {
  if constexpr (PAIR)
    return e.id;
  else
    return e.d >> (a.wide ? 9u : 8u);
}
template <bool PAIR, class Args>
OXC_DEV uint32_t entry_corner(const Args& a, const IdxEntry<PAIR>& e) {
  if constexpr (PAIR)
    return e.corner;
  else
    return e.d & ((1u << (a.wide ? 9u : 8u)) - 1u);
}

// k_draw_rows / k_vsm_draw_rows: the per-mesh-instance rows of the vertex fetch
template <class Args>
OXC_DEV void build_draw_rows(const Args& a) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.mesh_instance_count; i += gridDim.x * blockDim.x) {
    const GpuMeshInstance inst = a.mesh_instances[i];
    const GpuMesh* mesh = a.meshes + inst.mesh_index;
    const GpuMeshLOD* lod = reinterpret_cast<const GpuMeshLOD*>(mesh->lods) + inst.lod_index;
    DrawRow r;
    r.meshlets = lod->meshlets;
    r.micro = lod->local_triangle_indices;
    r.vidx = lod->indirect_vertex_indices;
    r.positions = mesh->vertex_positions;
    const float* wm = a.transforms + (size_t)inst.transform_index * 16;
#pragma unroll
    for (int rr = 0; rr < 3; rr++)
#pragma unroll
      for (int c = 0; c < 4; c++) r.w[rr * 4 + c] = OXC_M(wm, rr, c);
    a.rows[i] = r;
  }
}

// vs_main's fetch (visbuffer_encode.slang:24-49) for one corner: MeshletInstance -> DrawRow -> Meshlet record -> micro index -> vertex id
// -> dequantised position -> world position.  The three indices of a triangle written by cull_triangles name the same meshlet instance,
// so everything up to the Meshlet record and the world matrix is kept in `f` and reused while the instance id repeats (vs_main decodes
// every index on its own; an index list that mixes instances inside a triangle still works, slower).
struct CornerFetch {
  uint32_t mli_index = 0xFFFFFFFFu;
  uint4 ml = make_uint4(0, 0, 0, 0);  // {vertex_offset, tri_offset(bytes), vertex_count, tri_count}
  uint64_t micro = 0, vidx = 0, positions = 0;
  float w[12] = {0};  // rows 0..2 of world
};
// mli_rec: the instance's MeshletInstance record when the caller has fetched it already (k_draw_setup, a step ahead), else null
template <class Args>
OXC_DEV void corner_world(const Args& a, CornerFetch& f, uint32_t mli_index, uint32_t corner, const uint2* mli_rec, float (&world)[3]) {
  if (mli_index != f.mli_index) {
    f.mli_index = mli_index;
    const uint2 mli = mli_rec ? *mli_rec : reinterpret_cast<const uint2*>(a.meshlet_instances)[mli_index];
    const DrawRow* row = a.rows + mli.x;
    const uint4 p0 = reinterpret_cast<const uint4*>(row)[0], p1 = reinterpret_cast<const uint4*>(row)[1];
    const float4 w0 = reinterpret_cast<const float4*>(row)[2], w1 = reinterpret_cast<const float4*>(row)[3], w2 = reinterpret_cast<const float4*>(row)[4];
    f.micro = (uint64_t)p0.z | ((uint64_t)p0.w << 32);
    f.vidx = (uint64_t)p1.x | ((uint64_t)p1.y << 32);
    f.positions = (uint64_t)p1.z | ((uint64_t)p1.w << 32);
    f.ml = load_global_u4((uint64_t)p0.x | ((uint64_t)p0.y << 32), mli.y);
    f.w[0] = w0.x, f.w[1] = w0.y, f.w[2] = w0.z, f.w[3] = w0.w;
    f.w[4] = w1.x, f.w[5] = w1.y, f.w[6] = w1.z, f.w[7] = w1.w;
    f.w[8] = w2.x, f.w[9] = w2.y, f.w[10] = w2.z, f.w[11] = w2.w;
  }
  const uint32_t boff = f.ml.y + corner;
  const uint32_t li = (load_global_u32(f.micro, boff >> 2) >> ((boff & 3u) * 8u)) & 0xFFu;  // scene.slang:336-348
  const uint32_t vi = load_global_u32(f.vidx, f.ml.x + li);
  const uint2 q = load_global_u2(f.positions, vi);  // u16x4
  const float p[3] = {dequantize_half(q.x & 0xFFFFu), dequantize_half(q.x >> 16), dequantize_half(q.y & 0xFFFFu)};
#pragma unroll
  for (int r = 0; r < 3; r++) world[r] = ((f.w[r * 4 + 0] * p[0] + f.w[r * 4 + 1] * p[1]) + f.w[r * 4 + 2] * p[2]) + f.w[r * 4 + 3];
}

// mul(m, (p, 1)): the one projection_view multiply
OXC_DEV void mul_mp4(const float* m, const float* p, float* out) {
#pragma unroll
  for (int r = 0; r < 4; r++) out[r] = ((OXC_M(m, r, 0) * p[0] + OXC_M(m, r, 1) * p[1]) + OXC_M(m, r, 2) * p[2]) + OXC_M(m, r, 3);
}

// ---- edge functions, top-left rule, depth ----------------------------------------------------------------------------------------------
OXC_DEV int64_t edge_fn(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }
// The same edge function in 32-bit arithmetic: exact (no wrap) when every coordinate difference that enters it is below 2^15 in
// magnitude.  The 64-bit form is five emulated multi-word operations per edge on this hardware; pixels of the small path (corner
// spread < 2^12) and of most big-list tiles (< 2^15) qualify, and an exact integer is the same integer in either width.
OXC_DEV int32_t edge_fn32(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }
// top-left rule for positively oriented triangles: an edge owns its pixels when it goes down, or is horizontal going left
// (I = int32_t: coordinates are below 2^29 in magnitude, no wrap)
template <class I>
OXC_DEV bool edge_inclusive(I ax, I ay, I bx, I by) {
  const I dx = bx - ax, dy = by - ay;
  return dy > 0 || (dy == 0 && dx < 0);
}
// the pixel whose edge values (weights of corners 0, 1, 2) are e and whose edge biases (0: inclusive, -1: not) are b is covered
template <class I>
OXC_DEV bool covered(I e0, I e1, I e2, I b0, I b1, I b2) {
  return !(e0 + b0 < 0 || e1 + b1 < 0 || e2 + b2 < 0);
}
// z/w at a pixel: interpolated in binary64 from the exact edge values, one rounding to binary32
template <class I>
OXC_DEV float interpolate_depth(I e0, I e1, I e2, float z0, float z1, float z2, double inv_area) {
  const double zd = (((double)e0 * (double)z0 + (double)e1 * (double)z1) + (double)e2 * (double)z2) * inv_area;
  return (float)zd;
}

// ---- snap and setup --------------------------------------------------------------------------------------------------------------------
// The stated setup rules for one (possibly clipped) triangle given in clip coordinates, for a width x height viewport: out.x / y (24.8
// fixed point) and out.z, oriented with positive area.  Returns false when it is dropped: zero area, with CULL_BACK (cullMode eBack:
// det(xyw) > 0 <=> positive area) a back face (w <= 0 or a coordinate beyond the fixed-point range cannot happen behind the clipper
// but are kept as guards).
// spread: the larger of the corners' x and y extents (24.8 units); below 4096 every edge-function value of the triangle's own pixel box
// fits 32 bits with room to spare
template <bool CULL_BACK, class Out>
OXC_DEV bool setup_tri(float width, float height, const float* c0, const float* c1, const float* c2, Out& out, int32_t& spread) {
  const float* cl[3] = {c0, c1, c2};
  int32_t X[3], Y[3];  // |s| <= 2^20 pixels: the snapped values fit 32 bits (the stated rules are in integers; 64 bits are only needed for products)
  float z[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float* clip = cl[k];
    if (!(clip[3] > 0.0f)) return false;
    const float sx = ((clip[0] / clip[3]) * 0.5f + 0.5f) * width;
    const float sy = ((clip[1] / clip[3]) * 0.5f + 0.5f) * height;
    z[k] = clip[2] / clip[3];
    if (!(__builtin_fabsf(sx) <= 1048576.0f) || !(__builtin_fabsf(sy) <= 1048576.0f)) return false;
    X[k] = (int32_t)__builtin_floorf(sx * 256.0f + 0.5f);
    Y[k] = (int32_t)__builtin_floorf(sy * 256.0f + 0.5f);
  }
  spread = max(max(max(X[0], X[1]), X[2]) - min(min(X[0], X[1]), X[2]), max(max(Y[0], Y[1]), Y[2]) - min(min(Y[0], Y[1]), Y[2]));
  const int64_t area = spread < 32768 ? (int64_t)edge_fn32(X[0], Y[0], X[1], Y[1], X[2], Y[2]) : edge_fn(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
  if (area == 0 || (CULL_BACK && area > 0)) return false;
  const int o1 = area < 0 ? 2 : 1, o2 = area < 0 ? 1 : 2;  // negative area: swap corners 1 and 2
  out.x[0] = X[0], out.y[0] = Y[0], out.z[0] = z[0];
  out.x[1] = X[o1], out.y[1] = Y[o1], out.z[1] = z[o1];
  out.x[2] = X[o2], out.y[2] = Y[o2], out.z[2] = z[o2];
  return true;
}

// pixel box of an oriented setup, clamped to the width x height viewport; false when empty.  Pixel (px, py) has its centre at
// (256 px + 128, 256 py + 128).
template <class Tri>
OXC_DEV bool pixel_box(const Tri& t, int32_t width, int32_t height, int32_t& px0, int32_t& py0, int32_t& px1, int32_t& py1) {
  const int32_t minx = min(min(t.x[0], t.x[1]), t.x[2]), maxx = max(max(t.x[0], t.x[1]), t.x[2]);
  const int32_t miny = min(min(t.y[0], t.y[1]), t.y[2]), maxy = max(max(t.y[0], t.y[1]), t.y[2]);
  px0 = max((minx - 128 + 255) >> 8, 0);
  py0 = max((miny - 128 + 255) >> 8, 0);
  px1 = min((maxx - 128) >> 8, width - 1);
  py1 = min((maxy - 128) >> 8, height - 1);
  return px1 >= px0 && py1 >= py0;
}

// ---- the wave-level small-box pass -------------------------------------------------------------------------------------------------------
// Triangles whose pixel box is at most kSmallSpan x kSmallSpan with spread < 4096 are rasterised by their wave: the 64 boxes of a wave
// step are laid end to end (prefix sum of the box sizes) and every lane takes one box pixel per iteration, finding its triangle by a
// binary search over the 64 offsets in LDS.

// inclusive prefix sum across the 64 lanes
OXC_DEV uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// What a box pixel needs of its triangle, parked in LDS by the lane that set the triangle up (52 bytes; a pass that needs more per
// triangle keeps a record of its own with these fields: pack_small and wave_small_boxes take either)
struct SmallTri {
  int32_t x[3], y[3];
  float z[3];
  uint32_t inv_area_lo, inv_area_hi;
  uint32_t box;   // px0 | py0 << 16
  uint32_t misc;  // (box width - 1) | edge bias bits << 4 | ceil(256 / box width) << 8
};
constexpr bool small_division_exact() {  // k / bw == (k * ceil(256 / bw)) >> 8 for every box pixel index and width the small path sees
  for (int bw = 1; bw <= kSmallSpan; bw++)
    for (int k = 0; k < kSmallSpan * kSmallSpan; k++)
      if (k / bw != (k * ((256 + bw - 1) / bw)) >> 8) return false;
  return true;
}
static_assert(small_division_exact(), "box pixel index -> (x, y)");

// The packed words of oriented setup `t` whose pixel box starts at (px0, py0) and is bw <= kSmallSpan wide.  The caller copies the
// corners itself: with the copy in here k_draw_setup, which sits on its register limit, spilled 14 VGPRs where it spilled 5.
template <class Tri, class Small>
OXC_DEV void pack_small(const Tri& t, int32_t px0, int32_t py0, int32_t bw, Small& o) {
  const int32_t area = edge_fn32(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);  // > 0 (oriented), < 2^25
  const unsigned long long ia = __builtin_bit_cast(unsigned long long, 1.0 / (double)area);  // one reciprocal per triangle
  o.inv_area_lo = (uint32_t)ia;
  o.inv_area_hi = (uint32_t)(ia >> 32);
  o.box = (uint32_t)px0 | ((uint32_t)py0 << 16);
  const uint32_t bias = (edge_inclusive(t.x[1], t.y[1], t.x[2], t.y[2]) ? 0u : 1u) | (edge_inclusive(t.x[2], t.y[2], t.x[0], t.y[0]) ? 0u : 2u) |
                        (edge_inclusive(t.x[0], t.y[0], t.x[1], t.y[1]) ? 0u : 4u);
  o.misc = (uint32_t)(bw - 1) | (bias << 4) | (((256u + (uint32_t)bw - 1u) / (uint32_t)bw) << 8);
}

// The wave's small triangles, one box pixel per lane and iteration.  count: the box pixels of the record this lane parked in tl[lane]
// (0: none); tl, off: the wave's own LDS rows (T: SmallTri, or a record with its fields).  frag(q, e0, e1, e2, inv_area, px, py) is called for
// every covered box pixel with its triangle's record and its three 32-bit edge values.
template <class T, class F>
OXC_DEV void wave_small_boxes(const T* tl, uint32_t* off, uint32_t count, int lane, F&& frag) {
  const uint32_t incl = wave_incl_scan(count, lane);
  const uint32_t total = readlane_u(incl, 63);
  off[lane] = incl - count;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same-wave LDS hand-off: in order, no barrier needed
  for (uint32_t g0 = 0; g0 < total; g0 += 64u) {
    const uint32_t g = g0 + (uint32_t)lane;
    if (g < total) {
      uint32_t j = 0;  // the last triangle whose first box pixel is at or before g (empty boxes share their successor's offset)
#pragma unroll
      for (uint32_t stp = 32u; stp >= 1u; stp >>= 1)
        if (off[j + stp] <= g) j += stp;
      const uint32_t k = g - off[j];
      const T q = tl[j];
      const uint32_t bw = (q.misc & 7u) + 1u, m = q.misc >> 8;
      const uint32_t qy = (k * m) >> 8, qx = k - qy * bw;
      const uint32_t px = (q.box & 0xFFFFu) + qx, py = (q.box >> 16) + qy;
      const int32_t cx = (int32_t)px * 256 + 128, cy = (int32_t)py * 256 + 128;
      const int32_t e0 = edge_fn32(q.x[1], q.y[1], q.x[2], q.y[2], cx, cy);  // corner spread < 2^12, centre inside the box: |e| < 2^25
      const int32_t e1 = edge_fn32(q.x[2], q.y[2], q.x[0], q.y[0], cx, cy);
      const int32_t e2 = edge_fn32(q.x[0], q.y[0], q.x[1], q.y[1], cx, cy);
      if (covered(e0, e1, e2, (q.misc & 0x10u) ? -1 : 0, (q.misc & 0x20u) ? -1 : 0, (q.misc & 0x40u) ? -1 : 0)) {
        const double inv_area = __builtin_bit_cast(double, (unsigned long long)q.inv_area_lo | ((unsigned long long)q.inv_area_hi << 32));
        frag(q, e0, e1, e2, inv_area, px, py);
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the LDS rows are rewritten by the caller's next step
}

}  // namespace oxc
