// oxcull_vsm_draw.hip -- oxc_draw_physical_pages: the VSM shadow draw (gfx950).
//
// The tail of RendererInstance::draw_virtual_shadowmap (Shadowmaps.cpp:466-754): rmvsm_build_draw_commands and the indirect multi-draw
// of rmvsm_draw_physical_pages, as a compute rasteriser under the rules include/oxcull.h states (those of oxc_draw_visbuffer with cull
// mode None, a [0, 1] depth test, the fs_main page lookup and a u32 atomicMin per texel).  Its cost follows the dirty area:
//   k_vsm_draw_prologue  reads the page table once: the active clipmaps (descending), the optional commands, and per active clipmap a
//                        map virtual page -> physical page coords (all ones: not drawable), a bitmap of the drawable virtual pages and
//                        their bounding rectangle;
//   k_vsm_draw_rows      the per-mesh-instance rows of the vertex fetch (as oxc_draw_visbuffer's k_draw_rows);
//   k_vsm_draw_tris      one lane per triangle gathers its three world positions once, then loops over the active clipmaps: transform,
//                        screen box, page box; a pair whose page box holds no drawable page is dropped.  Pixel boxes up to 8 x 8 are
//                        rasterised by the wave (the visbuffer draw's box-distribution scheme), larger ones go to the big list,
//                        crossing triangles to the clip queue;
//   k_vsm_draw_clipped   the clipper for queued (triangle, clipmap) pairs, and an overflow pass that re-walks the list when the queue was full;
//   k_vsm_draw_big       one wave per big pair: its DRAWABLE pages (page box cut to the clipmap's drawable rectangle), drawn at once
//                        when at most kDirectPages, else one tile each;
//   k_vsm_draw_tiles     one wave per (pair, page) tile: the page's part of the pixel box;
//   k_vsm_draw_big_rescan  only when the big list overflowed: the big pairs beyond it, each drawn by a whole wave page by page.
// With no active clipmap every kernel returns after reading the active count.  The helpers below restate the visbuffer draw's
// arithmetic (oxcull_raster.hip) in this translation unit, which leaves that file's kernels untouched.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "oxcull_device.hpp"
#include "oxcull_kernels.hpp"

#pragma clang fp contract(off)

namespace oxc {
namespace {

constexpr int32_t kSmall = 8;           // pixel box side of the in-wave path
constexpr float kWMin = 0.0009765625f;  // 2^-10
constexpr float kGuard = 64.0f;
constexpr uint32_t kNoPage = 0xFFFFFFFFu;
// A big pair with at most this many drawable pages (page box within 64 pages) is drawn by the wave that found it; more go to the tile
// list.  Queueing every page made the first reference frame wait on one tile counter: 11.4 M returning atomics on one address, 129 ms.
constexpr uint32_t kDirectPages = 4;

// header words of the scratch (the counters on separate 128-byte lines)
// (zeroed in front of every call); H_RECT + 4 c: clipmap c's rectangle of drawable virtual pages as {n - min x, n - min y, max x + 1, max y + 1}
// (atomicMax from 0: all zero = no drawable page)
enum : uint32_t { H_ACTIVE = 0, H_LAYERS = 1, H_BIG = 32, H_TILES = 64, H_CLIP = 96, H_PAIRS = 128, H_FRAGS = 160, H_RECT = 192 };
static_assert(H_RECT + 4 * 16 <= kVsmDrawHeaderBytes / 4, "header");

OXC_DEV float clip_dist(const float* v, int plane) {
  switch (plane) {
    case 0: return v[3] - kWMin;
    case 1: return kGuard * v[3] - v[0];
    case 2: return kGuard * v[3] + v[0];
    case 3: return kGuard * v[3] - v[1];
    default: return kGuard * v[3] + v[1];
  }
}
OXC_DEV int64_t edge64(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }
OXC_DEV int32_t edge32(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }
// top-left rule for positively oriented triangles: an edge owns its pixels when it goes down, or is horizontal going left
OXC_DEV bool edge_incl(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  const int64_t dx = bx - ax, dy = by - ay;
  return dy > 0 || (dy == 0 && dx < 0);
}

OXC_DEV uint32_t active_count(const VsmDrawArgs& a) { return a.header[H_ACTIVE]; }

// VkDrawIndexedIndirectCommand: instanceCount 0 draws nothing; indices past the end of the buffer are not read
OXC_DEV uint32_t list_triangles(const VsmDrawArgs& a) { return a.draw_cmd[1] == 0u ? 0u : min(a.draw_cmd[0] / 3u, a.max_triangles); }

// 0: every corner inside every clip plane; 1: crosses a plane; 2: all corners outside one plane
OXC_DEV int clip_class(const float (&c)[3][4]) {
  bool crosses = false;
#pragma unroll
  for (int pl = 0; pl < 5; pl++) {
    const bool i0 = clip_dist(c[0], pl) >= 0.0f, i1 = clip_dist(c[1], pl) >= 0.0f, i2 = clip_dist(c[2], pl) >= 0.0f;
    if (!i0 && !i1 && !i2) return 2;
    crosses |= !(i0 && i1 && i2);
  }
  return crosses ? 1 : 0;
}

OXC_DEV void mul_mp4(const float* m, const float* p, float* out) {
#pragma unroll
  for (int r = 0; r < 4; r++) out[r] = ((OXC_M(m, r, 0) * p[0] + OXC_M(m, r, 1) * p[1]) + OXC_M(m, r, 2) * p[2]) + OXC_M(m, r, 3);
}

// vs_main's fetch for the three corners of triangle `tri`: world positions (Meshlet::index, Mesh::decode_position, world * (p, 1))
template <bool PAIR>
OXC_DEV void tri_world(const VsmDrawArgs& a, uint32_t tri, float (&world)[3][3]) {
  uint32_t cur = 0xFFFFFFFFu;
  uint4 ml = make_uint4(0, 0, 0, 0);
  uint64_t micro = 0, vidx = 0, positions = 0;
  float w[12] = {0};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    uint32_t mli_index, corner;
    if constexpr (PAIR) {
      const uint2 v = reinterpret_cast<const uint2*>(a.indices)[(size_t)tri * 3u + k];
      mli_index = v.x;
      corner = v.y;
    } else {
      const uint32_t d = a.indices[(size_t)tri * 3u + k];
      const uint32_t bits = a.wide ? 9u : 8u;
      mli_index = d >> bits;
      corner = d & ((1u << bits) - 1u);
    }
    if (mli_index != cur) {  // the three indices of a cull_triangles triangle share their meshlet instance
      cur = mli_index;
      const uint2 mli = reinterpret_cast<const uint2*>(a.meshlet_instances)[mli_index];
      const DrawRow* row = a.rows + mli.x;
      const uint4 p0 = reinterpret_cast<const uint4*>(row)[0], p1 = reinterpret_cast<const uint4*>(row)[1];
      const float4 w0 = reinterpret_cast<const float4*>(row)[2], w1 = reinterpret_cast<const float4*>(row)[3], w2 = reinterpret_cast<const float4*>(row)[4];
      micro = (uint64_t)p0.z | ((uint64_t)p0.w << 32);
      vidx = (uint64_t)p1.x | ((uint64_t)p1.y << 32);
      positions = (uint64_t)p1.z | ((uint64_t)p1.w << 32);
      ml = load_global_u4((uint64_t)p0.x | ((uint64_t)p0.y << 32), mli.y);  // {vertex_offset, tri_offset(bytes), vertex_count, tri_count}
      w[0] = w0.x, w[1] = w0.y, w[2] = w0.z, w[3] = w0.w;
      w[4] = w1.x, w[5] = w1.y, w[6] = w1.z, w[7] = w1.w;
      w[8] = w2.x, w[9] = w2.y, w[10] = w2.z, w[11] = w2.w;
    }
    const uint32_t boff = ml.y + corner;
    const uint32_t li = (load_global_u32(micro, boff >> 2) >> ((boff & 3u) * 8u)) & 0xFFu;  // scene.slang:336-348
    const uint32_t vi = load_global_u32(vidx, ml.x + li);
    const uint2 q = load_global_u2(positions, vi);  // u16x4
    const float p[3] = {dequantize_half(q.x & 0xFFFFu), dequantize_half(q.x >> 16), dequantize_half(q.y & 0xFFFFu)};
#pragma unroll
    for (int r = 0; r < 3; r++) world[k][r] = ((w[r * 4 + 0] * p[0] + w[r * 4 + 1] * p[1]) + w[r * 4 + 2] * p[2]) + w[r * 4 + 3];
  }
}

// The setup of one (possibly clipped) triangle with cull mode None: snapped corners, oriented with positive area.  False: zero area
// (or a guard that the clipper makes unreachable).
struct Setup {
  int32_t x[3], y[3];
  float z[3];
  int32_t spread;  // larger of the corners' x and y extents (24.8 units)
};
OXC_DEV bool setup_tri(float V, const float* c0, const float* c1, const float* c2, Setup& s) {
  const float* cl[3] = {c0, c1, c2};
  int32_t X[3], Y[3];  // |s| <= 2^20 pixels: the snapped values fit 32 bits
  float z[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float* c = cl[k];
    if (!(c[3] > 0.0f)) return false;
    const float sx = ((c[0] / c[3]) * 0.5f + 0.5f) * V;
    const float sy = ((c[1] / c[3]) * 0.5f + 0.5f) * V;
    z[k] = c[2] / c[3];
    if (!(__builtin_fabsf(sx) <= 1048576.0f) || !(__builtin_fabsf(sy) <= 1048576.0f)) return false;
    X[k] = (int32_t)__builtin_floorf(sx * 256.0f + 0.5f);
    Y[k] = (int32_t)__builtin_floorf(sy * 256.0f + 0.5f);
  }
  s.spread = max(max(max(X[0], X[1]), X[2]) - min(min(X[0], X[1]), X[2]), max(max(Y[0], Y[1]), Y[2]) - min(min(Y[0], Y[1]), Y[2]));
  const int64_t area = s.spread < 32768 ? (int64_t)edge32(X[0], Y[0], X[1], Y[1], X[2], Y[2]) : edge64(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
  if (area == 0) return false;
  const int o1 = area < 0 ? 2 : 1, o2 = area < 0 ? 1 : 2;  // negative area: swap corners 1 and 2
  s.x[0] = X[0], s.y[0] = Y[0], s.z[0] = z[0];
  s.x[1] = X[o1], s.y[1] = Y[o1], s.z[1] = z[o1];
  s.x[2] = X[o2], s.y[2] = Y[o2], s.z[2] = z[o2];
  return true;
}

// pixel box of an oriented setup, clamped to the V x V viewport; false when empty.  Pixel (px, py) has its centre at (256 px + 128, 256 py + 128).
OXC_DEV bool pixel_box(const Setup& s, int32_t V, int32_t& px0, int32_t& py0, int32_t& px1, int32_t& py1) {
  const int32_t minx = min(min(s.x[0], s.x[1]), s.x[2]), maxx = max(max(s.x[0], s.x[1]), s.x[2]);
  const int32_t miny = min(min(s.y[0], s.y[1]), s.y[2]), maxy = max(max(s.y[0], s.y[1]), s.y[2]);
  px0 = max((minx - 128 + 255) >> 8, 0);
  py0 = max((miny - 128 + 255) >> 8, 0);
  px1 = min((maxx - 128) >> 8, V - 1);
  py1 = min((maxy - 128) >> 8, V - 1);
  return px1 >= px0 && py1 >= py0;
}

OXC_DEV uint32_t page_of(const VsmDrawArgs& a, int32_t p) { return a.ps_shift >= 0 ? (uint32_t)p >> a.ps_shift : (uint32_t)p / a.page_size; }

OXC_DEV bool page_drawable(const VsmDrawArgs& a, uint32_t layer, uint32_t vx, uint32_t vy) {
  const uint32_t b = vy * a.n + vx;
  return (a.bitmap[(size_t)layer * a.words_per_layer + (b >> 5)] >> (b & 31u)) & 1u;
}

// the page box of pixel box [px0, px1] x [py0, py1] cut to the rectangle of `layer`'s drawable pages; false when that leaves nothing
OXC_DEV bool page_box(const VsmDrawArgs& a, uint32_t layer, int32_t px0, int32_t py0, int32_t px1, int32_t py1, uint32_t& qx0, uint32_t& qy0, uint32_t& qx1,
                      uint32_t& qy1) {
  const uint32_t* rc = a.header + H_RECT + 4u * layer;
  const int32_t n = (int32_t)a.n;
  const int32_t x0 = max((int32_t)page_of(a, px0), n - (int32_t)rc[0]), y0 = max((int32_t)page_of(a, py0), n - (int32_t)rc[1]);
  const int32_t x1 = min((int32_t)page_of(a, px1), (int32_t)rc[2] - 1), y1 = min((int32_t)page_of(a, py1), (int32_t)rc[3] - 1);
  qx0 = (uint32_t)x0, qy0 = (uint32_t)y0, qx1 = (uint32_t)x1, qy1 = (uint32_t)y1;
  return x1 >= x0 && y1 >= y0;
}

// does the page box of pixel box [px0, px1] x [py0, py1] hold a drawable page of `layer`?
OXC_DEV bool any_drawable(const VsmDrawArgs& a, uint32_t layer, int32_t px0, int32_t py0, int32_t px1, int32_t py1) {
  uint32_t qx0, qy0, qx1, qy1;
  if (!page_box(a, layer, px0, py0, px1, py1, qx0, qy0, qx1, qy1)) return false;
  const uint32_t* bm = a.bitmap + (size_t)layer * a.words_per_layer;
  for (uint32_t vy = qy0; vy <= qy1; vy++) {
    const uint32_t lo = vy * a.n + qx0, hi = vy * a.n + qx1;
    for (uint32_t w = lo >> 5; w <= (hi >> 5); w++) {
      const uint32_t first = w == (lo >> 5) ? (lo & 31u) : 0u, last = w == (hi >> 5) ? (hi & 31u) : 31u;
      const uint32_t mask = (0xFFFFFFFFu >> (31u - last)) & (0xFFFFFFFFu << first);
      if (bm[w] & mask) return true;
    }
  }
  return false;
}

// fs_main for one covered pixel: depth test, page lookup, atomicMin.  Returns 1 when it wrote.
OXC_DEV uint32_t fragment(const VsmDrawArgs& a, uint32_t layer, int64_t e0, int64_t e1, int64_t e2, const float* z, double inv_area, int32_t px, int32_t py) {
  const double zd = (((double)e0 * (double)z[0] + (double)e1 * (double)z[1]) + (double)e2 * (double)z[2]) * inv_area;
  const float zf = (float)zd;
  if (!(zf >= 0.0f) || zf > 1.0f) return 0u;
  const uint32_t vx = page_of(a, px), vy = page_of(a, py);
  const uint32_t m = a.pagemap[((size_t)layer * a.n + vy) * a.n + vx];
  if (m == kNoPage) return 0u;
  const uint32_t tx = (m & 0xFFFFu) * a.page_size + ((uint32_t)px - vx * a.page_size);
  const uint32_t ty = (m >> 16) * a.page_size + ((uint32_t)py - vy * a.page_size);
  atomicMin(reinterpret_cast<unsigned int*>(a.physical) + (size_t)ty * a.physical_size + tx, asu(zf));
  return 1u;
}

// what the per-pixel loop of a set-up triangle needs (64-bit edge values: exact for every coordinate the clipper lets through)
struct Raster {
  int64_t X[3], Y[3];
  float z[3];
  int64_t b[3];
  double inv_area;
  int32_t px0, py0, px1, py1;
  uint32_t layer;
};
OXC_DEV void prepare(const Setup& s, int32_t V, uint32_t layer, Raster& r) {
#pragma unroll
  for (int k = 0; k < 3; k++) r.X[k] = s.x[k], r.Y[k] = s.y[k], r.z[k] = s.z[k];
  r.b[0] = edge_incl(r.X[1], r.Y[1], r.X[2], r.Y[2]) ? 0 : -1;
  r.b[1] = edge_incl(r.X[2], r.Y[2], r.X[0], r.Y[0]) ? 0 : -1;
  r.b[2] = edge_incl(r.X[0], r.Y[0], r.X[1], r.Y[1]) ? 0 : -1;
  r.inv_area = 1.0 / (double)edge64(r.X[0], r.Y[0], r.X[1], r.Y[1], r.X[2], r.Y[2]);  // one reciprocal per triangle
  (void)pixel_box(s, V, r.px0, r.py0, r.px1, r.py1);
  r.layer = layer;
}
OXC_DEV uint32_t raster_pixel(const VsmDrawArgs& a, const Raster& r, int32_t px, int32_t py) {
  const int64_t cx = (int64_t)px * 256 + 128, cy = (int64_t)py * 256 + 128;
  const int64_t e0 = edge64(r.X[1], r.Y[1], r.X[2], r.Y[2], cx, cy);
  const int64_t e1 = edge64(r.X[2], r.Y[2], r.X[0], r.Y[0], cx, cy);
  const int64_t e2 = edge64(r.X[0], r.Y[0], r.X[1], r.Y[1], cx, cy);
  if (e0 + r.b[0] < 0 || e1 + r.b[1] < 0 || e2 + r.b[2] < 0) return 0u;
  return fragment(a, r.layer, e0, e1, e2, r.z, r.inv_area, px, py);
}
// one lane walks a pixel rectangle
OXC_DEV uint32_t walk_rect(const VsmDrawArgs& a, const Raster& r, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
  uint32_t n = 0;
  for (int32_t py = y0; py <= y1; py++)
    for (int32_t px = x0; px <= x1; px++) n += raster_pixel(a, r, px, py);
  return n;
}
// a wave walks a pixel rectangle in 8 x 8 blocks (lane = pixel of the block)
OXC_DEV uint32_t wave_rect(const VsmDrawArgs& a, const Raster& r, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int lane) {
  uint32_t n = 0;
  for (int32_t by = y0; by <= y1; by += 8)
    for (int32_t bx = x0; bx <= x1; bx += 8) {
      const int32_t px = bx + (lane & 7), py = by + (lane >> 3);
      if (px <= x1 && py <= y1) n += raster_pixel(a, r, px, py);
    }
  return n;
}
// the pixel rectangle of virtual page (vx, vy) inside the triangle's box
OXC_DEV bool page_rect(const VsmDrawArgs& a, const Raster& r, uint32_t vx, uint32_t vy, int32_t& x0, int32_t& y0, int32_t& x1, int32_t& y1) {
  const int32_t ps = (int32_t)a.page_size;
  x0 = max(r.px0, (int32_t)vx * ps);
  y0 = max(r.py0, (int32_t)vy * ps);
  x1 = min(r.px1, (int32_t)vx * ps + ps - 1);
  y1 = min(r.py1, (int32_t)vy * ps + ps - 1);
  return x1 >= x0 && y1 >= y0;
}

// A pair for the per-page path.  A pair the big list cannot hold is only counted: k_vsm_draw_big_rescan finds it again and draws it
// with the whole wave, page by page.
OXC_DEV void push_big(const VsmDrawArgs& a, const Setup& s, uint32_t layer) {
  const uint32_t slot = atomicAdd(a.header + H_BIG, 1u);
  if (slot >= a.big_capacity) return;
  VsmBig b;
#pragma unroll
  for (int k = 0; k < 3; k++) b.x[k] = s.x[k], b.y[k] = s.y[k], b.z[k] = s.z[k];
  b.layer = layer;
  a.big_list[slot] = b;
}

// The drawable pages of a pair's page box, walked by the whole wave (`r` is wave-uniform): lanes test 64 pages at a time, then the wave
// rasterises each drawable one.
OXC_DEV uint32_t wave_pages(const VsmDrawArgs& a, const Raster& r, int lane) {
  uint32_t qx0, qy0, qx1, qy1;
  if (!page_box(a, r.layer, r.px0, r.py0, r.px1, r.py1, qx0, qy0, qx1, qy1)) return 0u;
  const uint32_t qw = qx1 - qx0 + 1u, np = qw * (qy1 - qy0 + 1u);
  uint32_t n = 0;
  for (uint32_t k0 = 0; k0 < np; k0 += 64u) {  // wave-uniform
    const uint32_t k = k0 + (uint32_t)lane;
    const uint32_t vy = qy0 + k / qw, vx = qx0 + k % qw;
    uint64_t pages = __builtin_amdgcn_ballot_w64(k < np && page_drawable(a, r.layer, vx, vy));
    while (pages) {
      const int l = __builtin_ctzll(pages);
      pages &= pages - 1ull;
      int32_t x0, y0, x1, y1;
      if (page_rect(a, r, readlane_u(vx, l), readlane_u(vy, l), x0, y0, x1, y1)) n += wave_rect(a, r, x0, y0, x1, y1, lane);
    }
  }
  return n;
}

template <bool STATS>
OXC_DEV void add_stats(const VsmDrawArgs& a, uint32_t pairs, uint32_t frags) {
  if constexpr (STATS) {
    if (pairs) atomicAdd(a.header + H_PAIRS, pairs);
    if (frags) atomicAdd(a.header + H_FRAGS, frags);
  }
}

// a small-box triangle parked in LDS for the wave's box-distribution pass
struct SmallLds {
  int32_t x[3], y[3];
  float z[3];
  uint32_t inv_area_lo, inv_area_hi;
  uint32_t box;   // px0 | py0 << 16
  uint32_t misc;  // (box width - 1) | edge bias bits << 4 | ceil(256 / box width) << 8
};

}  // namespace

__global__ __launch_bounds__(256) void k_vsm_draw_prologue(VsmDrawArgs a) {
  const uint32_t layer = blockIdx.y;
  if (blockIdx.x == 0 && layer == 0 && threadIdx.x == 0) {  // rmvsm_build_draw_commands: one thread, as the reference dispatches it
    uint32_t cnt = 0;
    for (int c = (int)a.layers - 1; c >= 0; c--) {
      if (a.dirty_flags[c] == 0u) continue;
      a.header[H_LAYERS + cnt] = (uint32_t)c;
      if (a.out_clipmaps) {
        a.out_clipmaps[cnt] = (uint32_t)c;
        for (uint32_t w = 0; w < 5u; w++) a.out_cmds[cnt * 5u + w] = a.draw_cmd[w];
      }
      cnt++;
    }
    a.header[H_ACTIVE] = cnt;
    if (a.out_count) *a.out_count = cnt;
  }
  if (a.dirty_flags[layer] == 0u) return;
  // this clipmap's page_offset reduced into [0, n): wrapped = v + off, minus n when that reaches n (= floor_mod(v + page_offset, n))
  const int32_t* rec = reinterpret_cast<const int32_t*>(a.clipmaps + (size_t)layer * 19u);
  const int32_t n = (int32_t)a.n;
  const uint32_t offx = (uint32_t)(((rec[16] % n) + n) % n), offy = (uint32_t)(((rec[17] % n) + n) % n);
  const uint32_t P = a.phys_side, pages = a.phys_side * a.phys_side;
  const uint32_t* table = a.page_table + (size_t)layer * a.n * a.n;
  uint32_t lo_x = 0, lo_y = 0, hi_x = 0, hi_y = 0;  // this thread's part of the drawable rectangle, in H_RECT's encoding
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < a.words_per_layer; w += gridDim.x * blockDim.x) {
    uint32_t bits = 0;
    for (uint32_t k = 0; k < 32u; k++) {
      const uint32_t b = w * 32u + k, vy = b / a.n, vx = b - vy * a.n;
      uint32_t wx = vx + offx, wy = vy + offy;
      wx -= wx >= a.n ? a.n : 0u;
      wy -= wy >= a.n ? a.n : 0u;
      const uint32_t e = table[wy * a.n + wx];
      const uint32_t addr = e >> 16;
      const bool ok = (e & 6u) == 6u && addr < pages;  // Backed (4) && Dirty (2), an address inside the image
      a.pagemap[(size_t)layer * a.n * a.n + b] = ok ? ((addr % P) | ((addr / P) << 16)) : kNoPage;
      bits |= ok ? (1u << k) : 0u;
      if (ok) {
        lo_x = max(lo_x, a.n - vx), lo_y = max(lo_y, a.n - vy);
        hi_x = max(hi_x, vx + 1u), hi_y = max(hi_y, vy + 1u);
      }
    }
    a.bitmap[(size_t)layer * a.words_per_layer + w] = bits;
  }
  if (hi_x) {
    uint32_t* rc = a.header + H_RECT + 4u * layer;
    atomicMax(rc + 0, lo_x);
    atomicMax(rc + 1, lo_y);
    atomicMax(rc + 2, hi_x);
    atomicMax(rc + 3, hi_y);
  }
}

__global__ __launch_bounds__(256) void k_vsm_draw_rows(VsmDrawArgs a) {
  if (active_count(a) == 0u) return;
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

template <bool PAIR, bool STATS>
__global__ __launch_bounds__(256) void k_vsm_draw_tris(VsmDrawArgs a) {
  const uint32_t count = active_count(a);
  if (count == 0u) return;  // nothing dirty: the index list is not walked
  set_half_denorm_flush();
  __shared__ float s_pv[16][16];
  __shared__ uint32_t s_layer[16];
  __shared__ SmallLds s_tri[4][64];
  __shared__ uint32_t s_off[4][64];
  for (uint32_t i = threadIdx.x; i < count * 16u; i += blockDim.x) {
    const uint32_t layer = a.header[H_LAYERS + i / 16u];
    s_pv[i / 16u][i % 16u] = a.clipmaps[(size_t)layer * 19u + (i % 16u)];
    if (i % 16u == 0u) s_layer[i / 16u] = layer;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  SmallLds* const tl = s_tri[wave];
  uint32_t* const off = s_off[wave];
  const uint32_t tris = list_triangles(a);
  const uint32_t wave_id = blockIdx.x * 4u + (uint32_t)wave, nwaves = gridDim.x * 4u;
  const int32_t V = (int32_t)a.V;
  const float Vf = (float)a.V;
  uint32_t pairs = 0, frags = 0;
  for (uint32_t base = wave_id * 64u; base < tris; base += nwaves * 64u) {  // wave-uniform
    const uint32_t tri = base + (uint32_t)lane;
    const bool valid = tri < tris;
    float world[3][3] = {};
    if (valid) tri_world<PAIR>(a, tri, world);
    for (uint32_t slot = 0; slot < count; slot++) {  // wave-uniform
      const uint32_t layer = s_layer[slot];
      uint32_t cnt = 0;
      if (valid) {
        float clip[3][4];
#pragma unroll
        for (int k = 0; k < 3; k++) mul_mp4(s_pv[slot], world[k], clip[k]);
        const int cls = clip_class(clip);
        Setup s;
        int32_t px0, py0, px1, py1;
        if (cls == 1) {  // rare: crosses w = 2^-10 or the guard band -- k_vsm_draw_clipped, one thread per pair
          const uint32_t q = atomicAdd(a.header + H_CLIP, 1u);
          if (q < a.clip_capacity) a.clip_list[q] = make_uint2(tri, layer);
        } else if (cls == 0 && setup_tri(Vf, clip[0], clip[1], clip[2], s) && pixel_box(s, V, px0, py0, px1, py1) &&
                   any_drawable(a, layer, px0, py0, px1, py1)) {
          pairs++;
          const int32_t bw = px1 - px0 + 1, bh = py1 - py0 + 1;
          if (bw <= kSmall && bh <= kSmall && s.spread < 4096) {
            cnt = (uint32_t)(bw * bh);
            SmallLds o;
#pragma unroll
            for (int k = 0; k < 3; k++) o.x[k] = s.x[k], o.y[k] = s.y[k], o.z[k] = s.z[k];
            const int32_t area = edge32(s.x[0], s.y[0], s.x[1], s.y[1], s.x[2], s.y[2]);  // > 0 (oriented), < 2^25
            const unsigned long long ia = __builtin_bit_cast(unsigned long long, 1.0 / (double)area);
            o.inv_area_lo = (uint32_t)ia;
            o.inv_area_hi = (uint32_t)(ia >> 32);
            o.box = (uint32_t)px0 | ((uint32_t)py0 << 16);
            const uint32_t bias = (edge_incl(s.x[1], s.y[1], s.x[2], s.y[2]) ? 0u : 1u) | (edge_incl(s.x[2], s.y[2], s.x[0], s.y[0]) ? 0u : 2u) |
                                  (edge_incl(s.x[0], s.y[0], s.x[1], s.y[1]) ? 0u : 4u);
            o.misc = (uint32_t)(bw - 1) | (bias << 4) | (((256u + (uint32_t)bw - 1u) / (uint32_t)bw) << 8);
            tl[lane] = o;
          } else {
            push_big(a, s, layer);
          }
        }
      }
      // the wave's small boxes laid end to end, one box pixel per lane and iteration (the visbuffer draw's scheme)
      uint32_t incl = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      const uint32_t total = readlane_u(incl, 63);
      off[lane] = incl - cnt;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same-wave LDS hand-off: in order, no block barrier needed
      for (uint32_t g0 = 0; g0 < total; g0 += 64u) {
        const uint32_t g = g0 + (uint32_t)lane;
        if (g < total) {
          uint32_t j = 0;  // the last triangle whose first box pixel is at or before g (empty boxes share their successor's offset)
#pragma unroll
          for (uint32_t stp = 32u; stp >= 1u; stp >>= 1)
            if (off[j + stp] <= g) j += stp;
          const uint32_t k = g - off[j];
          const SmallLds q = tl[j];
          const uint32_t bw = (q.misc & 7u) + 1u, m = q.misc >> 8;
          const uint32_t qy = (k * m) >> 8, qx = k - qy * bw;
          const int32_t px = (int32_t)((q.box & 0xFFFFu) + qx), py = (int32_t)((q.box >> 16) + qy);
          const int32_t cx = px * 256 + 128, cy = py * 256 + 128;
          const int32_t e0 = edge32(q.x[1], q.y[1], q.x[2], q.y[2], cx, cy);  // corner spread < 2^12, centre inside the box: |e| < 2^25
          const int32_t e1 = edge32(q.x[2], q.y[2], q.x[0], q.y[0], cx, cy);
          const int32_t e2 = edge32(q.x[0], q.y[0], q.x[1], q.y[1], cx, cy);
          if (e0 + ((q.misc & 0x10u) ? -1 : 0) >= 0 && e1 + ((q.misc & 0x20u) ? -1 : 0) >= 0 && e2 + ((q.misc & 0x40u) ? -1 : 0) >= 0) {
            const double inv_area = __builtin_bit_cast(double, (unsigned long long)q.inv_area_lo | ((unsigned long long)q.inv_area_hi << 32));
            frags += fragment(a, layer, e0, e1, e2, q.z, inv_area, px, py);
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the LDS rows are rewritten by the next clipmap
    }
  }
  add_stats<STATS>(a, pairs, frags);
}

// Sutherland-Hodgman against the five planes, fan triangulation, then the same setup as an unclipped pair (oxc_draw_visbuffer's
// clipper: a new vertex goes from the inside end I to the outside end O, so neighbours share it).  RESCAN: the queue overflowed and the
// pairs beyond it were not recorded -- walk every (triangle, active clipmap) pair again and clip the crossing ones (drawing a pair twice
// leaves the image unchanged: atomicMin).  Returns at once when the queue did not overflow.
template <bool RESCAN, bool PAIR, bool STATS>
__global__ __launch_bounds__(64) void k_vsm_draw_clipped(VsmDrawArgs a) {
  const uint32_t count = active_count(a);
  if (count == 0u) return;
  const uint32_t queued = a.header[H_CLIP];
  if (RESCAN && queued <= a.clip_capacity) return;
  set_half_denorm_flush();
  const uint64_t items = RESCAN ? (uint64_t)list_triangles(a) * count : (uint64_t)min(queued, a.clip_capacity);
  const int32_t V = (int32_t)a.V;
  uint32_t pairs = 0, frags = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t tri, layer;
    if (RESCAN) {
      tri = (uint32_t)(i / count);
      layer = a.header[H_LAYERS + (uint32_t)(i % count)];
    } else {
      const uint2 it = a.clip_list[i];
      tri = it.x;
      layer = it.y;
    }
    float world[3][3];
    tri_world<PAIR>(a, tri, world);
    const float* pv = a.clipmaps + (size_t)layer * 19u;
    float poly[2][9][4];
    float c3[3][4];
    for (int k = 0; k < 3; k++) {
      mul_mp4(pv, world[k], c3[k]);
      for (int c = 0; c < 4; c++) poly[0][k][c] = c3[k][c];
    }
    if (RESCAN && clip_class(c3) != 1) continue;
    int nv = 3, cur = 0;
    for (int pl = 0; pl < 5 && nv >= 3; pl++) {
      int m = 0;
      for (int k = 0; k < nv; k++) {
        const float* p = poly[cur][k];
        const float* q = poly[cur][(k + 1) % nv];
        const float dp = clip_dist(p, pl), dq = clip_dist(q, pl);
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
      nv = m;
      cur ^= 1;
    }
    for (int k = 1; k + 1 < nv; k++) {
      Setup s;
      int32_t px0, py0, px1, py1;
      if (!setup_tri((float)a.V, poly[cur][0], poly[cur][k], poly[cur][k + 1], s) || !pixel_box(s, V, px0, py0, px1, py1) ||
          !any_drawable(a, layer, px0, py0, px1, py1))
        continue;
      pairs++;
      if (px1 - px0 < kSmall && py1 - py0 < kSmall) {
        Raster r;
        prepare(s, V, layer, r);
        frags += walk_rect(a, r, r.px0, r.py0, r.px1, r.py1);
      } else {
        push_big(a, s, layer);
      }
    }
  }
  add_stats<STATS>(a, pairs, frags);
}

// One wave per big pair: it draws the drawable pages of its page box itself when they are few, else hands out a tile per drawable page
// (lanes over the pages, one atomic per 64 pages).  Tiles that do not fit the tile list are walked by this wave.
template <bool STATS>
__global__ __launch_bounds__(256) void k_vsm_draw_big(VsmDrawArgs a) {
  if (active_count(a) == 0u) return;
  const uint32_t total = min(a.header[H_BIG], a.big_capacity);
  const int lane = threadIdx.x & 63;
  const uint32_t wave_id = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
  uint32_t frags = 0;
  for (uint32_t i = wave_id; i < total; i += nwaves) {  // wave-uniform
    const VsmBig b = a.big_list[i];
    Setup s;
#pragma unroll
    for (int k = 0; k < 3; k++) s.x[k] = b.x[k], s.y[k] = b.y[k], s.z[k] = b.z[k];
    Raster r;
    prepare(s, (int32_t)a.V, b.layer, r);
    uint32_t qx0, qy0, qx1, qy1;  // (the page box cut to the layer's drawable rectangle)
    if (!page_box(a, b.layer, r.px0, r.py0, r.px1, r.py1, qx0, qy0, qx1, qy1)) continue;
    const uint32_t qw = qx1 - qx0 + 1u, np = qw * (qy1 - qy0 + 1u);
    for (uint32_t k0 = 0; k0 < np; k0 += 64u) {  // wave-uniform
      const uint32_t k = k0 + (uint32_t)lane;
      const uint32_t vy = qy0 + k / qw, vx = qx0 + k % qw;
      const bool mine = k < np && page_drawable(a, b.layer, vx, vy);
      const uint64_t ballot = __builtin_amdgcn_ballot_w64(mine);
      if (ballot == 0) continue;
      if (np <= 64u && (uint32_t)__builtin_popcountll(ballot) <= kDirectPages) {  // a few pages (nearly every big pair): drawn here, no queue atomic
        uint64_t pages = ballot;
        while (pages) {
          const int l = __builtin_ctzll(pages);
          pages &= pages - 1ull;
          int32_t x0, y0, x1, y1;
          if (page_rect(a, r, readlane_u(vx, l), readlane_u(vy, l), x0, y0, x1, y1)) frags += wave_rect(a, r, x0, y0, x1, y1, lane);
        }
        continue;
      }
      uint32_t first = 0;
      if (lane == 0) first = atomicAdd(a.header + H_TILES, (uint32_t)__builtin_popcountll(ballot));
      first = readlane_u(first, 0);
      const uint32_t rank = (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
      const bool fits = first + rank < a.tile_capacity && first + rank >= first;
      if (mine && fits) a.tile_list[first + rank] = make_uint2(i, vy * a.n + vx);
      uint64_t spill = __builtin_amdgcn_ballot_w64(mine && !fits);
      while (spill) {  // wave-uniform: the tile list is full, this wave walks the tiles itself
        const int l = __builtin_ctzll(spill);
        spill &= spill - 1ull;
        const uint32_t sx = readlane_u(vx, l), sy = readlane_u(vy, l);
        int32_t x0, y0, x1, y1;
        if (page_rect(a, r, sx, sy, x0, y0, x1, y1)) frags += wave_rect(a, r, x0, y0, x1, y1, lane);
      }
    }
  }
  add_stats<STATS>(a, 0u, frags);
}

// One wave per (big pair, drawable page) tile.
template <bool STATS>
__global__ __launch_bounds__(256) void k_vsm_draw_tiles(VsmDrawArgs a) {
  if (active_count(a) == 0u) return;
  const uint32_t count = min(a.header[H_TILES], a.tile_capacity);
  const int lane = threadIdx.x & 63;
  const uint32_t wave_id = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
  uint32_t frags = 0;
  for (uint32_t i = wave_id; i < count; i += nwaves) {  // wave-uniform
    const uint2 item = a.tile_list[i];
    const VsmBig b = a.big_list[item.x];
    Setup s;
#pragma unroll
    for (int k = 0; k < 3; k++) s.x[k] = b.x[k], s.y[k] = b.y[k], s.z[k] = b.z[k];
    Raster r;
    prepare(s, (int32_t)a.V, b.layer, r);
    int32_t x0, y0, x1, y1;
    if (page_rect(a, r, item.y % a.n, item.y / a.n, x0, y0, x1, y1)) frags += wave_rect(a, r, x0, y0, x1, y1, lane);
  }
  add_stats<STATS>(a, 0u, frags);
}

// Overflow pass of the big list: more big pairs than it holds (the count went on past big_capacity), and the ones beyond it were not
// recorded.  Every (triangle, active clipmap) pair is set up again -- clipped when it crosses a plane -- and every big one is drawn by the
// whole wave over its drawable pages; pairs the list did hold are drawn a second time, which leaves the image unchanged (atomicMin).
// Returns at once when the list did not overflow.
template <bool PAIR, bool STATS>
__global__ __launch_bounds__(256) void k_vsm_draw_big_rescan(VsmDrawArgs a) {
  const uint32_t count = active_count(a);
  if (count == 0u || a.header[H_BIG] <= a.big_capacity) return;
  set_half_denorm_flush();
  const int lane = threadIdx.x & 63;
  const uint32_t tris = list_triangles(a);
  const uint32_t wave_id = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
  const int32_t V = (int32_t)a.V;
  uint32_t frags = 0;
  for (uint32_t base = wave_id * 64u; base < tris; base += nwaves * 64u) {  // wave-uniform
    const uint32_t tri = base + (uint32_t)lane;
    const bool valid = tri < tris;
    float world[3][3] = {};
    if (valid) tri_world<PAIR>(a, tri, world);
    for (uint32_t slot = 0; slot < count; slot++) {  // wave-uniform
      const uint32_t layer = a.header[H_LAYERS + slot];
      const float* pv = a.clipmaps + (size_t)layer * 19u;
      float poly[2][9][4];
      float c3[3][4];
      for (int k = 0; k < 3; k++) {
        mul_mp4(pv, world[k], c3[k]);
        for (int c = 0; c < 4; c++) poly[0][k][c] = c3[k][c];
      }
      const int cls = valid ? clip_class(c3) : 2;
      int nv = cls == 2 ? 0 : 3, cur = 0;
      if (cls == 1) {  // the clipper of k_vsm_draw_clipped
        for (int pl = 0; pl < 5 && nv >= 3; pl++) {
          int m = 0;
          for (int k = 0; k < nv; k++) {
            const float* p = poly[cur][k];
            const float* q = poly[cur][(k + 1) % nv];
            const float dp = clip_dist(p, pl), dq = clip_dist(q, pl);
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
          nv = m;
          cur ^= 1;
        }
      }
      for (int k = 1; k < 8; k++) {  // fan triangle k of every lane's polygon (wave-uniform bound: at most 9 corners)
        Setup s = {};
        int32_t px0 = 0, py0 = 0, px1 = -1, py1 = -1;
        // big: every pair push_big received (k_vsm_draw_tris: box beyond 8 x 8 or spread >= 4096; k_vsm_draw_clipped: box beyond 8 x 8)
        const bool big = k + 1 < nv && setup_tri((float)a.V, poly[cur][0], poly[cur][k], poly[cur][k + 1], s) && pixel_box(s, V, px0, py0, px1, py1) &&
                         !(px1 - px0 < kSmall && py1 - py0 < kSmall && s.spread < 4096) && any_drawable(a, layer, px0, py0, px1, py1);
        uint64_t lanes = __builtin_amdgcn_ballot_w64(big);
        while (lanes) {  // wave-uniform: one lane's pair at a time, drawn by the whole wave
          const int l = __builtin_ctzll(lanes);
          lanes &= lanes - 1ull;
          Setup u;
#pragma unroll
          for (int c = 0; c < 3; c++) {
            u.x[c] = (int32_t)readlane_u((uint32_t)s.x[c], l);
            u.y[c] = (int32_t)readlane_u((uint32_t)s.y[c], l);
            u.z[c] = readlane_f(asu(s.z[c]), l);
          }
          Raster r;
          prepare(u, V, layer, r);
          frags += wave_pages(a, r, lane);
        }
      }
    }
  }
  add_stats<STATS>(a, 0u, frags);
}

template <bool PAIR, bool STATS>
static void launch_draw(const VsmDrawArgs& a, uint32_t max_grid, hipStream_t s) {
  hipLaunchKernelGGL((k_vsm_draw_tris<PAIR, STATS>), dim3(max_grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL((k_vsm_draw_clipped<false, PAIR, STATS>), dim3(std::min(256u, max_grid)), dim3(64), 0, s, a);
  hipLaunchKernelGGL((k_vsm_draw_clipped<true, PAIR, STATS>), dim3(max_grid), dim3(64), 0, s, a);  // (returns at once unless the queue overflowed)
  hipLaunchKernelGGL((k_vsm_draw_big<STATS>), dim3(max_grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL((k_vsm_draw_tiles<STATS>), dim3(max_grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL((k_vsm_draw_big_rescan<PAIR, STATS>), dim3(max_grid), dim3(256), 0, s, a);  // (returns at once unless the big list overflowed)
}

void launch_vsm_draw(const VsmDrawArgs& a, bool stats, uint32_t max_grid, hipStream_t s) {
  const uint32_t gx = std::max(1u, std::min((a.words_per_layer + 255u) / 256u, max_grid));
  (void)hipMemsetAsync(a.header, 0, kVsmDrawHeaderBytes, s);  // counters and rectangles (the prologue writes the active list)
  hipLaunchKernelGGL(k_vsm_draw_prologue, dim3(gx, a.layers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_vsm_draw_rows, dim3(std::max(1u, std::min((a.mesh_instance_count + 255u) / 256u, max_grid))), dim3(256), 0, s, a);
  if (a.wide == 2u) {
    if (stats)
      launch_draw<true, true>(a, max_grid, s);
    else
      launch_draw<true, false>(a, max_grid, s);
  } else {
    if (stats)
      launch_draw<false, true>(a, max_grid, s);
    else
      launch_draw<false, false>(a, max_grid, s);
  }
}

}  // namespace oxc
