// oxcull_sprites.hip -- the 2D pass (gfx950): sprites and particles drawn over the lit image between oxc_apply_pbr and oxc_apply_fxaa
// (RendererInstance.cpp:1080-1223; shaders passes/2d_forward_vis.slang, passes/2d_forward.slang, editor/mouse_picking_2d.slang).  Rules:
// include/oxcull.h, oxc_draw_sprites (S1 - S7); design and measurements: DESIGN.md section 29.
//
// Sprites are the one draw of the library whose fragments depend on their order: several translucent sprites over one pixel must run depth
// test, depth write and blend in the order of the sorted list.  The order is built without a lock and without an atomic:
//   k_sprites_setup   one lane per sprite: S1 - S3, the clip class and setup_tri<false> of its triangles.  The usual sprite -- two
//                     triangles inside every plane -- fills a 128-byte record; a sprite that crosses a plane goes through clip_polygon and
//                     puts up to twelve fan triangles into the side array at its own index.  Discarded, dropped and empty sprites get an
//                     empty pixel box.
//   k_sprites_bin     one block per kSpriteBin x kSpriteBin pixel bin walks the boxes in order, kSpriteChunk a step, and appends the
//                     sprites that meet the bin to the bin's list by ballot and prefix count: the list is ascending by construction.  A
//                     bin that meets more than kSpriteBinCapacity sprites only counts them.
//   k_sprites_pixels  one block per kSpriteTile x kSpriteTile tile, one pixel per lane.  It compacts its bin's list (or, for a bin that
//                     overflowed, the whole sprite range) against the tile the same way into LDS, a chunk at a time, and every lane
//                     walks the chunk in order with its depth, its visbuffer word and its colour word in registers: S4 - S7.  Both
//                     stages of a call run in this one launch over the same bins, the vis stage over the whole list first.  Depth,
//                     visbuffer and colour are read once and written once per pixel (not at all in a tile no sprite meets).
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction.
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"
#include "oxcull_raster_device.hpp"

namespace oxc {
namespace {
constexpr uint32_t kEmptyBoxLo = 0xFFFFFFFFu;
static_assert(sizeof(SpriteTri) == 48 && sizeof(SpriteRecord) == 128, "record layout");
static_assert(kSpriteChunk == 256 && kSpriteTile * kSpriteTile == 256, "one sprite, one pixel per lane of a 256-lane block");
static_assert(kSpriteBin % kSpriteTile == 0, "a tile lies in one bin");
// a tile that meets a sprite's pixel box lies within kSpriteTile px of its corners' box: below 2^15 units with the narrow spread
static_assert(kSpriteNarrowSpread + (int32_t)kSpriteTile * 256 <= 32768, "edge_fn32 is exact for narrow sprites");

// The block's ordered compaction step: the position of this lane's item among the block's hits, `total` their number.  The caller
// synchronises the block before the next step reuses s_wave.
OXC_DEV uint32_t block_rank(bool hit, uint32_t* s_wave, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t b = __ballot(hit);
  if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t before = 0u;
  total = 0u;
#pragma unroll
  for (uint32_t k = 0u; k < 4u; k++) {
    const uint32_t c = s_wave[k];
    before += k < wave ? c : 0u;
    total += c;
  }
  return before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

// the pixel box `box` meets the pixel rectangle [x0, x0 + side) x [y0, y0 + side)
OXC_DEV bool box_meets(uint2 box, uint32_t x0, uint32_t y0, uint32_t side) {
  const uint32_t bx0 = box.x & 0xFFFFu, by0 = box.x >> 16, bx1 = box.y & 0xFFFFu, by1 = box.y >> 16;
  return bx0 < x0 + side && bx1 >= x0 && by0 < y0 + side && by1 >= y0;  // the empty box has bx0 = 0xFFFF, beyond every extent
}

// S4 for one triangle at the pixel centre (cx, cy): covered, and its depth in (0, 1]
template <class I>
OXC_DEV bool tri_fragment(const SpriteTri& t, int32_t cx, int32_t cy, float& d) {
  I e0, e1, e2;
  if constexpr (sizeof(I) == 4) {
    e0 = edge_fn32(t.x[1], t.y[1], t.x[2], t.y[2], cx, cy);
    e1 = edge_fn32(t.x[2], t.y[2], t.x[0], t.y[0], cx, cy);
    e2 = edge_fn32(t.x[0], t.y[0], t.x[1], t.y[1], cx, cy);
  } else {
    e0 = edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], cx, cy);
    e1 = edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], cx, cy);
    e2 = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], cx, cy);
  }
  if (!covered<I>(e0, e1, e2, (t.bias & 1u) ? -1 : 0, (t.bias & 2u) ? -1 : 0, (t.bias & 4u) ? -1 : 0)) return false;
  const double inv_area = __builtin_bit_cast(double, (unsigned long long)t.inv_area_lo | ((unsigned long long)t.inv_area_hi << 32));
  d = interpolate_depth(e0, e1, e2, t.z[0], t.z[1], t.z[2], inv_area);
  return d > 0.0f && !(d > 1.0f);
}

// S6 on the stored words of one pixel: decode, blend, store
template <int FORMAT>
OXC_DEV void blend(uint32_t& c0, uint32_t& c1, const float* ca, float a, float oma) {
  if (FORMAT == 0) {
    const float r = ca[0] + unpack_ufloat<6>(c0 & 0x7FFu) * oma, g = ca[1] + unpack_ufloat<6>((c0 >> 11) & 0x7FFu) * oma, b = ca[2] + unpack_ufloat<5>(c0 >> 22) * oma;
    c0 = pack_ufloat<6>(r) | (pack_ufloat<6>(g) << 11) | (pack_ufloat<5>(b) << 22);
  } else {
    const float r = ca[0] + dequantize_half(c0 & 0xFFFFu) * oma, g = ca[1] + dequantize_half(c0 >> 16) * oma, b = ca[2] + dequantize_half(c1 & 0xFFFFu) * oma;
    const float al = a + dequantize_half(c1 >> 16) * oma;
    c0 = channel_half(r) | (channel_half(g) << 16);
    c1 = channel_half(b) | (channel_half(al) << 16);
  }
}
}  // namespace

__global__ __launch_bounds__(256) void k_sprites_setup(SpriteArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.sprite_count) return;
  const uint32_t w0 = a.sprites[(size_t)i * 3u], w1 = a.sprites[(size_t)i * 3u + 1u], transform_id = a.sprites[(size_t)i * 3u + 2u];
  a.boxes[i] = make_uint2(kEmptyBoxLo, 0u);
  if (transform_id >= a.transform_count) return;  // S1, stated: dropped whole

  // S1, S2: the material's words (all zero beyond material_count), the colour, the discard
  const uint32_t flags = w1 & 0xFFFFu, material_index = w0 & 0xFFFFu;
  uint32_t m0 = 0u, m1 = 0u, m4 = 0u;
  if (material_index < a.material_count) {
    const uint32_t* rec = a.materials + (size_t)material_index * 14u;
    m0 = rec[0], m1 = rec[1], m4 = rec[4];
  }
  const float color[4] = {dequantize_half_flush(m0 & 0xFFFFu), dequantize_half_flush(m0 >> 16), dequantize_half_flush(m1 & 0xFFFFu), dequantize_half_flush(m1 >> 16)};
  if (color[3] <= dequantize_half_flush(m4 >> 16)) return;

  // S3: the four distinct corners; the triangles are (0, 1, 2) and (2, 3, 0)
  const float* wm = a.transforms + (size_t)transform_id * 16u;
  const float fx = (flags & 2u) ? -1.0f : 1.0f;
  const float cornerx[4] = {-0.5f * fx, 0.5f * fx, 0.5f * fx, -0.5f * fx}, cornery[4] = {-0.5f, -0.5f, 0.5f, 0.5f};
  float clip[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float world[3];
#pragma unroll
    for (int r = 0; r < 3; r++) world[r] = ((OXC_M(wm, r, 0) * cornerx[k] + OXC_M(wm, r, 1) * cornery[k]) + OXC_M(wm, r, 2) * 0.0f) + OXC_M(wm, r, 3);
    mul_mp4(a.pv, world, clip[k]);
  }
  const int corner_of[2][3] = {{0, 1, 2}, {2, 3, 0}};
  int cls[2];
#pragma unroll
  for (int t = 0; t < 2; t++) {
    float tc[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int c = 0; c < 4; c++) tc[k][c] = clip[corner_of[t][k]][c];
    cls[t] = tri_clip_class(tc);
  }
  const bool clipped = cls[0] == 1 || cls[1] == 1;
  SpriteRecord* const rec = a.records + i;
  SpriteTri* const dst = clipped ? a.clipped + (size_t)i * kSpriteMaxTris : rec->tri;

  // S4: setup of every triangle; the sprite's pixel box and its corners' box
  uint32_t n = 0u;
  int32_t bx0 = 0x7FFFFFFF, by0 = 0x7FFFFFFF, bx1 = -1, by1 = -1;
  int32_t cx0 = 0x7FFFFFFF, cy0 = 0x7FFFFFFF, cx1 = -0x7FFFFFFF, cy1 = -0x7FFFFFFF;
  const float fw = (float)a.w, fh = (float)a.h;
  auto emit = [&](const float* c0, const float* c1, const float* c2) {
    SpriteTri t;
    int32_t spread, px0, py0, px1, py1;
    if (!setup_tri<false>(fw, fh, c0, c1, c2, t, spread)) return;
    if (!pixel_box(t, (int32_t)a.w, (int32_t)a.h, px0, py0, px1, py1)) return;  // no pixel centre: no fragment
    const int64_t area = spread < 32768 ? (int64_t)edge_fn32(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]) : edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
    const unsigned long long ia = __builtin_bit_cast(unsigned long long, 1.0 / (double)area);
    t.inv_area_lo = (uint32_t)ia, t.inv_area_hi = (uint32_t)(ia >> 32);
    t.bias = (edge_inclusive(t.x[1], t.y[1], t.x[2], t.y[2]) ? 0u : 1u) | (edge_inclusive(t.x[2], t.y[2], t.x[0], t.y[0]) ? 0u : 2u) |
             (edge_inclusive(t.x[0], t.y[0], t.x[1], t.y[1]) ? 0u : 4u);
    dst[n++] = t;
    bx0 = min(bx0, px0), by0 = min(by0, py0), bx1 = max(bx1, px1), by1 = max(by1, py1);
#pragma unroll
    for (int k = 0; k < 3; k++) cx0 = min(cx0, t.x[k]), cx1 = max(cx1, t.x[k]), cy0 = min(cy0, t.y[k]), cy1 = max(cy1, t.y[k]);
  };
  for (int t = 0; t < 2; t++) {
    if (cls[t] == 2) continue;
    if (cls[t] == 0) {
      emit(clip[corner_of[t][0]], clip[corner_of[t][1]], clip[corner_of[t][2]]);
    } else {
      float poly[2][9][4];
      for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) poly[0][k][c] = clip[corner_of[t][k]][c];
      int cur;
      const int corners = clip_polygon(poly, cur);
      for (int k = 1; k + 1 < corners; k++) emit(poly[cur][0], poly[cur][k], poly[cur][k + 1]);
    }
  }
  if (n == 0u) return;
  const bool narrow = cx1 - cx0 < kSpriteNarrowSpread && cy1 - cy0 < kSpriteNarrowSpread;
  rec->ca[0] = color[0] * color[3], rec->ca[1] = color[1] * color[3], rec->ca[2] = color[2] * color[3];
  rec->a = color[3], rec->one_minus_a = 1.0f - color[3];
  rec->transform_id = transform_id;
  rec->shape = n | (clipped ? 0x100u : 0u) | (narrow ? 0x200u : 0u);
  a.boxes[i] = make_uint2((uint32_t)bx0 | ((uint32_t)by0 << 16), (uint32_t)bx1 | ((uint32_t)by1 << 16));
}

__global__ __launch_bounds__(256) void k_sprites_bin(SpriteArgs a) {
  __shared__ uint32_t s_wave[4];
  const uint32_t bin = blockIdx.x, x0 = (bin % a.bins_x) * kSpriteBin, y0 = (bin / a.bins_x) * kSpriteBin;
  uint32_t* const list = a.bin_lists + (size_t)bin * a.list_stride;
  uint32_t count = 0u;
  for (uint32_t base = 0u; base < a.sprite_count; base += kSpriteChunk) {
    const uint32_t j = base + threadIdx.x;
    const bool hit = j < a.sprite_count && box_meets(a.boxes[j], x0, y0, kSpriteBin);
    uint32_t hits;
    const uint32_t at = count + block_rank(hit, s_wave, hits);
    if (hit && at < a.list_stride) list[at] = j;
    count += hits;
    __syncthreads();
  }
  if (threadIdx.x == 0u) a.bin_counts[bin] = count;
}

template <int FORMAT>
__global__ __launch_bounds__(256) void k_sprites_pixels(SpriteArgs a) {
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_list[kSpriteChunk];
  const uint32_t tiles_x = (a.w + kSpriteTile - 1u) / kSpriteTile;
  const uint32_t x0 = (blockIdx.x % tiles_x) * kSpriteTile, y0 = (blockIdx.x / tiles_x) * kSpriteTile;
  const uint32_t px = x0 + (threadIdx.x & (kSpriteTile - 1u)), py = y0 + threadIdx.x / kSpriteTile;
  const bool inside = px < a.w && py < a.h;
  const size_t pix = (size_t)py * a.w + px;
  const bool vis_stage = (a.stages & 1u) != 0u, color_stage = (a.stages & 2u) != 0u;
  const bool clear = vis_stage && a.clear != 0u;

  const uint32_t bin = (y0 / kSpriteBin) * a.bins_x + x0 / kSpriteBin;
  const uint32_t bin_count = a.bin_counts[bin];
  const bool whole = bin_count > a.list_stride;  // the bin's list overflowed: walk the sprite range itself (slower, the same order)
  const uint32_t sources = whole ? a.sprite_count : bin_count;
  const uint32_t* const list = a.bin_lists + (size_t)bin * a.list_stride;

  bool loaded = false, dirty = false;
  float depth = 0.0f;
  uint32_t vis = ~0u, c0 = 0u, c1 = 0u;
  const int32_t cx = (int32_t)px * 256 + 128, cy = (int32_t)py * 256 + 128;

  for (uint32_t stage = 1u; stage <= 2u; stage <<= 1) {
    if (!(a.stages & stage)) continue;
    for (uint32_t base = 0u; base < sources; base += kSpriteChunk) {
      const uint32_t j = base + threadIdx.x;
      uint32_t index = 0u;
      bool hit = false;
      if (j < sources) {
        index = whole ? j : list[j];
        hit = box_meets(a.boxes[index], x0, y0, kSpriteTile);
      }
      uint32_t hits;
      const uint32_t at = block_rank(hit, s_wave, hits);
      if (hit) s_list[at] = index;
      __syncthreads();
      if (hits != 0u && !loaded) {  // block-uniform
        loaded = true;
        if (inside) {
          depth = a.depth[pix];
          if (vis_stage && !clear) vis = a.vis[pix];
          if (color_stage) {
            if (FORMAT == 0) {
              c0 = static_cast<const uint32_t*>(a.color)[pix];
            } else {
              const uint2 v = static_cast<const uint2*>(a.color)[pix];
              c0 = v.x, c1 = v.y;
            }
          }
        }
      }
      for (uint32_t k = 0u; k < hits; k++) {
        const uint32_t si = readfirst_u(s_list[k]);
        const SpriteRecord* const rec = a.records + si;
        const uint32_t shape = rec->shape;
        const SpriteTri* const tris = (shape & 0x100u) ? a.clipped + (size_t)si * kSpriteMaxTris : rec->tri;
        const bool narrow = (shape & 0x200u) != 0u;
        for (uint32_t t = 0u; t < (shape & 0xFFu); t++) {
          const SpriteTri q = tris[t];
          float d = 0.0f;
          const bool fragment = narrow ? tri_fragment<int32_t>(q, cx, cy, d) : tri_fragment<int64_t>(q, cx, cy, d);
          if (inside && fragment && d >= depth) {  // S5
            depth = d;
            dirty = true;
            if (stage == 1u)
              vis = rec->transform_id;
            else
              blend<FORMAT>(c0, c1, rec->ca, rec->a, rec->one_minus_a);
          }
        }
      }
      __syncthreads();  // s_list and s_wave are rewritten by the next step
    }
  }

  if (!inside) return;
  if (dirty) {
    a.depth[pix] = depth;
    if (color_stage) {
      if (FORMAT == 0)
        static_cast<uint32_t*>(a.color)[pix] = c0;
      else
        static_cast<uint2*>(a.color)[pix] = make_uint2(c0, c1);
    }
  }
  if (vis_stage && (dirty || clear)) a.vis[pix] = vis;
}

__global__ void k_pick_sprite(const uint32_t* vis, uint32_t w, uint32_t x, uint32_t y, uint32_t* out) {
  if (threadIdx.x == 0u) out[0] = vis[(size_t)y * w + x];
}

void launch_draw_sprites(const SpriteArgs& a, uint32_t format, hipStream_t s) {
  hipLaunchKernelGGL(k_sprites_setup, dim3((a.sprite_count + 255u) / 256u), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sprites_bin, dim3(a.bins_x * a.bins_y), dim3(256), 0, s, a);
  const uint32_t tiles = ((a.w + kSpriteTile - 1u) / kSpriteTile) * ((a.h + kSpriteTile - 1u) / kSpriteTile);  // at most 2^20
  if (format == 0u)
    hipLaunchKernelGGL(k_sprites_pixels<0>, dim3(tiles), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_sprites_pixels<1>, dim3(tiles), dim3(256), 0, s, a);
}

void launch_pick_sprite(const uint32_t* vis, uint32_t w, uint32_t x, uint32_t y, uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_pick_sprite, dim3(1), dim3(64), 0, s, vis, w, x, y, out);
}

}  // namespace oxc
