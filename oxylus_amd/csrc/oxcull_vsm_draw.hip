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
// With no active clipmap every kernel returns after reading the active count.  The rasteriser arithmetic -- clip planes and clipper,
// index decode and vertex fetch, row builder, snap, pixel box, edge functions, top-left rule, depth interpolation and the wave's
// box-distribution pass -- is oxcull_raster_device.hpp's, the one copy this draw shares with oxc_draw_visbuffer.  What is written here is
// what differs: cull mode None, the [0, 1] depth test, the page lookup and atomicMin, the page bitmap and rectangle, the per-page
// big path and the statistics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "oxcull_raster_device.hpp"

#pragma clang fp contract(off)

namespace oxc {
namespace {

constexpr uint32_t kNoPage = 0xFFFFFFFFu;
// A big pair with at most this many drawable pages (page box within 64 pages) is drawn by the wave that found it; more go to the tile
// list.  Queueing every page made the first reference frame wait on one tile counter: 11.4 M returning atomics on one address, 129 ms.
constexpr uint32_t kDirectPages = 4;

// header words of the scratch (the counters on separate 128-byte lines)
// (zeroed in front of every call); H_RECT + 4 c: clipmap c's rectangle of drawable virtual pages as {n - min x, n - min y, max x + 1, max y + 1}
// (atomicMax from 0: all zero = no drawable page)
enum : uint32_t { H_ACTIVE = 0, H_LAYERS = 1, H_BIG = 32, H_TILES = 64, H_CLIP = 96, H_PAIRS = 128, H_FRAGS = 160, H_RECT = 192 };
static_assert(H_RECT + 4 * 16 <= kVsmDrawHeaderBytes / 4, "header");

OXC_DEV uint32_t active_count(const VsmDrawArgs& a) { return a.header[H_ACTIVE]; }

// VkDrawIndexedIndirectCommand: instanceCount 0 draws nothing; indices past the end of the buffer are not read
OXC_DEV uint32_t list_triangles(const VsmDrawArgs& a) { return a.draw_cmd[1] == 0u ? 0u : min(a.draw_cmd[0] / 3u, a.max_triangles); }

// vs_main's fetch for the three corners of triangle `tri`: world positions (Meshlet::index, Mesh::decode_position, world * (p, 1))
template <bool PAIR>
OXC_DEV void tri_world(const VsmDrawArgs& a, uint32_t tri, float (&world)[3][3]) {
  CornerFetch f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const IdxEntry<PAIR> e = load_entry<PAIR>(a, (size_t)tri * 3u + k);
    corner_world(a, f, entry_instance<PAIR>(a, e), entry_corner<PAIR>(a, e), nullptr, world[k]);
  }
}

// The setup of one (possibly clipped) triangle (setup_tri, cull mode None): snapped corners, oriented with positive area
struct Setup {
  int32_t x[3], y[3];
  float z[3];
  int32_t spread;  // larger of the corners' x and y extents (24.8 units)
};
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
template <class I>
OXC_DEV uint32_t fragment(const VsmDrawArgs& a, uint32_t layer, I e0, I e1, I e2, const float* z, double inv_area, int32_t px, int32_t py) {
  const float zf = interpolate_depth(e0, e1, e2, z[0], z[1], z[2], inv_area);
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
  r.b[0] = edge_inclusive(r.X[1], r.Y[1], r.X[2], r.Y[2]) ? 0 : -1;
  r.b[1] = edge_inclusive(r.X[2], r.Y[2], r.X[0], r.Y[0]) ? 0 : -1;
  r.b[2] = edge_inclusive(r.X[0], r.Y[0], r.X[1], r.Y[1]) ? 0 : -1;
  r.inv_area = 1.0 / (double)edge_fn(r.X[0], r.Y[0], r.X[1], r.Y[1], r.X[2], r.Y[2]);  // one reciprocal per triangle
  (void)pixel_box(s, V, V, r.px0, r.py0, r.px1, r.py1);
  r.layer = layer;
}
OXC_DEV uint32_t raster_pixel(const VsmDrawArgs& a, const Raster& r, int32_t px, int32_t py) {
  const int64_t cx = (int64_t)px * 256 + 128, cy = (int64_t)py * 256 + 128;
  const int64_t e0 = edge_fn(r.X[1], r.Y[1], r.X[2], r.Y[2], cx, cy);
  const int64_t e1 = edge_fn(r.X[2], r.Y[2], r.X[0], r.Y[0], cx, cy);
  const int64_t e2 = edge_fn(r.X[0], r.Y[0], r.X[1], r.Y[1], cx, cy);
  if (!covered(e0, e1, e2, r.b[0], r.b[1], r.b[2])) return 0u;
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
  build_draw_rows(a);
}

template <bool PAIR, bool STATS>
__global__ __launch_bounds__(256) void k_vsm_draw_tris(VsmDrawArgs a) {
  const uint32_t count = active_count(a);
  if (count == 0u) return;  // nothing dirty: the index list is not walked
  set_half_denorm_flush();
  __shared__ float s_pv[16][16];
  __shared__ uint32_t s_layer[16];
  __shared__ SmallTri s_tri[4][64];
  __shared__ uint32_t s_off[4][64];
  for (uint32_t i = threadIdx.x; i < count * 16u; i += blockDim.x) {
    const uint32_t layer = a.header[H_LAYERS + i / 16u];
    s_pv[i / 16u][i % 16u] = a.clipmaps[(size_t)layer * 19u + (i % 16u)];
    if (i % 16u == 0u) s_layer[i / 16u] = layer;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  SmallTri* const tl = s_tri[wave];
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
        const int cls = tri_clip_class(clip);
        Setup s;
        int32_t px0, py0, px1, py1;
        if (cls == 1) {  // rare: crosses w = 2^-10 or the guard band -- k_vsm_draw_clipped, one thread per pair
          const uint32_t q = atomicAdd(a.header + H_CLIP, 1u);
          if (q < a.clip_capacity) a.clip_list[q] = make_uint2(tri, layer);
        } else if (cls == 0 && setup_tri<false>(Vf, Vf, clip[0], clip[1], clip[2], s, s.spread) && pixel_box(s, V, V, px0, py0, px1, py1) &&
                   any_drawable(a, layer, px0, py0, px1, py1)) {
          pairs++;
          const int32_t bw = px1 - px0 + 1, bh = py1 - py0 + 1;
          if (bw <= kSmallSpan && bh <= kSmallSpan && s.spread < 4096) {
            cnt = (uint32_t)(bw * bh);
            SmallTri o;
#pragma unroll
            for (int k = 0; k < 3; k++) o.x[k] = s.x[k], o.y[k] = s.y[k], o.z[k] = s.z[k];
            pack_small(s, px0, py0, bw, o);
            tl[lane] = o;
          } else {
            push_big(a, s, layer);
          }
        }
      }
      // the wave's small boxes laid end to end, one box pixel per lane and iteration
      wave_small_boxes(tl, off, cnt, lane, [&](const SmallTri& q, int32_t e0, int32_t e1, int32_t e2, double inv_area, uint32_t px, uint32_t py) {
        frags += fragment(a, layer, e0, e1, e2, q.z, inv_area, (int32_t)px, (int32_t)py);
      });
    }
  }
  add_stats<STATS>(a, pairs, frags);
}

// The clipper (clip_polygon), fan triangulation, then the same setup as an unclipped pair.  RESCAN: the queue overflowed and the
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
    if (RESCAN && tri_clip_class(c3) != 1) continue;
    int cur;
    const int nv = clip_polygon(poly, cur);
    for (int k = 1; k + 1 < nv; k++) {
      Setup s;
      int32_t px0, py0, px1, py1;
      if (!setup_tri<false>((float)a.V, (float)a.V, poly[cur][0], poly[cur][k], poly[cur][k + 1], s, s.spread) || !pixel_box(s, V, V, px0, py0, px1, py1) ||
          !any_drawable(a, layer, px0, py0, px1, py1))
        continue;
      pairs++;
      if (px1 - px0 < kSmallSpan && py1 - py0 < kSmallSpan) {
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
      const int cls = valid ? tri_clip_class(c3) : 2;
      int nv = cls == 2 ? 0 : 3, cur = 0;
      if (cls == 1) nv = clip_polygon(poly, cur);
      for (int k = 1; k < 8; k++) {  // fan triangle k of every lane's polygon (wave-uniform bound: at most 9 corners)
        Setup s = {};
        int32_t px0 = 0, py0 = 0, px1 = -1, py1 = -1;
        // big: every pair push_big received (k_vsm_draw_tris: box beyond 8 x 8 or spread >= 4096; k_vsm_draw_clipped: box beyond 8 x 8)
        const bool big = k + 1 < nv && setup_tri<false>((float)a.V, (float)a.V, poly[cur][0], poly[cur][k], poly[cur][k + 1], s, s.spread) && pixel_box(s, V, V, px0, py0, px1, py1) &&
                         !(px1 - px0 < kSmallSpan && py1 - py0 < kSmallSpan && s.spread < 4096) && any_drawable(a, layer, px0, py0, px1, py1);
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
