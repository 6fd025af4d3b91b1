// oxcull_highlight.hip -- the editor's selection path (gfx950): the click that asks which entity lies under the cursor and the outline around
// the selected entities (OxylusEditor/src/Panels/ViewportPanel.cpp:1166-1556; shaders editor/mouse_picking.slang, highlight_mask.slang,
// highlight_dilate_horizontal.slang, highlight_composite.slang).  Rules: include/oxcull.h, oxc_pick_transform and oxc_apply_highlight (P, M1 -
// M2, H1 - H5); design and measurements: DESIGN.md section 28.
//
//   k_pick_transform        one lane: rule P of one texel.
//   k_highlight_mask        one wave per 64 consecutive pixels of a row, four waves a block.  Each lane resolves its texel's transform; the wave
//                           then takes the distinct transforms it holds one at a time (neighbouring pixels mostly share one) and tests
//                           each against the selection list 64 entries a step, one entry per lane and one ballot per step: the list is read
//                           once per wave and distinct transform, not once per lane.  The ballot of the results is the row's mask word, stored
//                           by lane 0.
//   k_highlight_composite   one block per 64 x 16 pixel tile (one mask word wide).  The mask is one bit per pixel and a dilation is a maximum
//                           over zeros and ones, so both dilations run on words: the block dilates the word column of every row the tile's
//                           window reaches horizontally into LDS -- the word itself smeared by shift-and-OR doubling; of a neighbouring word
//                           only its nearest set bit matters, which one count-zeros finds -- then ORs the window's rows per output row, sixteen
//                           lanes a row.  A wave then walks four rows of 64 pixels; a pixel that is no edge and has alpha byte 255 is a copy of
//                           its word (H5), so depth is loaded and the float path run for the outline's pixels and for translucent ones only.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction.
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {
namespace {
constexpr uint32_t kTileRows = 16, kMaxRadius = 255;

// P: the transform index behind a visbuffer texel
OXC_DEV uint32_t texel_transform(const HighlightRecords& r, uint32_t texel) {
  if (texel == ~0u) return ~0u;
  const uint32_t instance = texel >> 8;
  if (instance == kTerrainInstanceId) return r.terrain_transform_index;
  if (instance >= r.meshlet_instance_count) return 0u;  // the all-zero MeshInstance; nothing is loaded
  return r.mesh_instances[r.meshlet_instances[instance].mesh_instance_index].transform_index;
}

// word k of a mask row without the bits past the image's width
OXC_DEV uint64_t mask_word(const uint64_t* row, uint32_t k, uint32_t words, uint32_t w) {
  const uint64_t v = row[k];
  const uint32_t tail = w & 63u;
  return (k + 1u == words && tail) ? v & ((1ull << tail) - 1ull) : v;
}

// the OR of v shifted by -r .. r bits, r <= 63: each step doubles the run of shifts already covered
OXC_DEV uint64_t smear(uint64_t v, uint32_t r) {
  uint64_t up = v, down = v;
  for (uint32_t covered = 0u; covered < r;) {
    const uint32_t step = min(covered + 1u, r - covered);  // at most 32
    up |= up << step;
    down |= down >> step;
    covered += step;
  }
  return up | down;
}

// H1, horizontal: bit q of the result is set when the row holds a mask bit within rx pixels of pixel 64 * k + q
OXC_DEV uint64_t dilate_row(const uint64_t* row, uint32_t k, uint32_t words, uint32_t w, uint32_t rx) {
  uint64_t out = smear(mask_word(row, k, words, w), min(rx, 63u));
  const uint32_t reach = (rx + 63u) / 64u;  // words on each side that can hold such a bit
  for (uint32_t d = 1u; d <= reach; d++) {
    if (k + d < words) {  // to the right: its lowest bit reaches furthest, down to pixel q = lo
      const uint64_t s = mask_word(row, k + d, words, w);
      const int lo = (int)(64u * d) + __builtin_ctzll(s | (1ull << 63)) - (int)rx;
      if (s && lo <= 63) out |= lo <= 0 ? ~0ull : ~0ull << lo;
    }
    if (k >= d) {  // to the left: its highest bit, up to pixel q = hi
      const uint64_t s = mask_word(row, k - d, words, w);
      const int hi = (63 - __builtin_clzll(s | 1ull)) - (int)(64u * d) + (int)rx;
      if (s && hi >= 0) out |= hi >= 63 ? ~0ull : ~0ull >> (63 - hi);
    }
  }
  return out;
}
}  // namespace

__global__ void k_pick_transform(PickArgs a) {
  if (threadIdx.x == 0u) a.out[0] = texel_transform(a.r, a.r.vis[(size_t)a.y * a.r.w + a.x]);
}

__global__ __launch_bounds__(256) void k_highlight_mask(HighlightMaskArgs a) {
  const uint32_t lane = threadIdx.x & 63u, words = (a.r.w + 63u) / 64u;
  const uint64_t item = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);  // the wave's word of the image
  if (item >= (uint64_t)words * a.r.h) return;                           // the whole wave leaves
  const uint32_t y = (uint32_t)(item / words), k = (uint32_t)(item - (uint64_t)y * words);
  const uint32_t x = k * 64u + lane;
  const bool inside = x < a.r.w;
  const size_t pix = (size_t)y * a.r.w + x;
  const uint32_t transform = inside ? texel_transform(a.r, a.r.vis[pix]) : ~0u;

  // M1: the wave's distinct transforms, one at a time
  bool selected = false;
  uint64_t todo = a.selected_count ? __ballot(transform != ~0u) : 0ull;
  while (todo) {
    const uint32_t u = __shfl(transform, (int)__builtin_ctzll(todo));  // never ~0u: no padding lane and no ~0u entry equals it
    bool hit = false;
    for (uint32_t base = 0u; base < a.selected_count && !hit; base += 64u) {
      const uint32_t i = base + lane;
      hit = __ballot((i < a.selected_count ? a.selected[i] : ~0u) == u) != 0ull;
    }
    const bool mine = transform == u;
    if (mine) selected = hit;
    todo &= ~__ballot(mine);
  }

  // M2
  const uint64_t bits = __ballot(selected);
  if (lane == 0u) a.mask_bits[item] = bits;
  if (a.mask_attachment && inside) a.mask_attachment[pix] = selected ? 255u : 0u;
}

__global__ __launch_bounds__(256) void k_highlight_composite(HighlightCompositeArgs a) {
  __shared__ uint64_t s_row[kTileRows + 2u * kMaxRadius];  // the word column of every row of the window, dilated horizontally
  __shared__ uint64_t s_mask[kTileRows], s_dilated[kTileRows];
  const uint32_t tid = threadIdx.x, words = (a.w + 63u) / 64u;
  const uint32_t k = blockIdx.x % words, y0 = (blockIdx.x / words) * kTileRows;
  const uint32_t rows = min(kTileRows, a.h - y0);
  const uint32_t lo = y0 > a.ry ? y0 - a.ry : 0u, hi = min(a.h - 1u, y0 + rows - 1u + a.ry);  // H1: the window cut to the image

  for (uint32_t i = tid; i <= hi - lo; i += 256u) {
    const uint32_t y = lo + i;
    const uint64_t* row = a.mask_bits + (size_t)y * words;
    s_row[i] = dilate_row(row, k, words, a.w, a.rx);
    if (y >= y0 && y < y0 + rows) s_mask[y - y0] = mask_word(row, k, words, a.w);
  }
  __syncthreads();

  // H1, vertical: sixteen lanes OR the rows of one output row's window
  {
    const uint32_t t = tid >> 4, part = tid & 15u;
    uint64_t acc = 0ull;
    if (t < rows) {
      const uint32_t y = y0 + t;
      const uint32_t first = (y > a.ry ? max(lo, y - a.ry) : lo) - lo, last = min(hi, y + a.ry) - lo;
      for (uint32_t j = first + part; j <= last; j += 16u) acc |= s_row[j];
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) acc |= __shfl_xor(acc, m);
    if (part == 0u && t < rows) s_dilated[t] = acc;
  }
  __syncthreads();

  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t x = k * 64u + lane;
  if (x >= a.w) return;
  const bool srgb = a.format != 2u;
  for (uint32_t r = 0u; r < 4u; r++) {
    const uint32_t t = wave * 4u + r;
    if (t >= rows) break;
    const size_t pix = (size_t)(y0 + t) * a.w + x;
    const uint32_t word = a.color[pix];
    const bool edge = (((s_dilated[t] & ~s_mask[t]) >> lane) & 1ull) != 0ull;  // H2
    if (!edge && (word >> 24) == 0xFFu) {  // H5: decode, blend and store give the same four bytes
      a.dst[pix] = word;
      continue;
    }
    // H3, in the order of the word's bytes (a.outline is in that order too)
    float src[4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const uint32_t byte = (word >> (8 * c)) & 0xFFu;
      src[c] = srgb ? srgb_decode(byte) : (float)byte / 255.0f;
    }
    src[3] = (float)(word >> 24) / 255.0f;
    if (edge) {  // H4
      const bool occluded = a.depth[pix] > 0.00001f;
      if (occluded && a.occluded_mode == 1) {
#pragma unroll
        for (int c = 0; c < 4; c++) src[c] = src[c] + (a.outline[c] - src[c]) * 0.35f;
      } else if (!(occluded && a.occluded_mode == 0)) {
#pragma unroll
        for (int c = 0; c < 4; c++) src[c] = a.outline[c];
      }
    }
    // H5
    uint32_t out = pack_unorm(src[3] + (1.0f - src[3])) << 24;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float v = src[c] * src[3];
      out |= pack_unorm(srgb ? srgb_encode(v) : v) << (8 * c);
    }
    a.dst[pix] = out;
  }
}

// H4: srgb_to_linear of common/color.slang:75-77 on the three colour channels, the alpha as given
void highlight_outline_linear(const float* outline_color, float* final_outline) {
  for (int c = 0; c < 3; c++) {
    const float v = outline_color[c];
    final_outline[c] = v < 0.04045f ? v / 12.92f : pow_rule_host(std::fabs(v + 0.055f) / 1.055f, 2.4f);
  }
  final_outline[3] = outline_color[3];
}

void launch_pick_transform(const PickArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_pick_transform, dim3(1), dim3(64), 0, s, a); }

void launch_highlight_mask(const HighlightMaskArgs& a, hipStream_t s) {
  const uint64_t items = (uint64_t)((a.r.w + 63u) / 64u) * a.r.h;  // at most 2^26
  hipLaunchKernelGGL(k_highlight_mask, dim3((uint32_t)((items + 3u) / 4u)), dim3(256), 0, s, a);
}

void launch_highlight_composite(const HighlightCompositeArgs& a, hipStream_t s) {
  const uint32_t tiles = ((a.w + 63u) / 64u) * ((a.h + kTileRows - 1u) / kTileRows);  // at most 2^22
  hipLaunchKernelGGL(k_highlight_composite, dim3(tiles), dim3(256), 0, s, a);
}

}  // namespace oxc
