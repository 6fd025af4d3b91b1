// oxcull_fxaa.hip -- edge anti-aliasing of the lit HDR image (gfx950): the `fxaa` pass of the reference's post-process chain
// (Oxylus/src/Render/Shaders/passes/fxaa/fxaa.slang, bound at RendererInstance.cpp:1225-1255).  Rules: include/oxcull.h, oxc_apply_fxaa;
// design and measurements: DESIGN.md section 20.
//
//   k_fxaa   one thread per pixel from tile_pixel(), a 16 x 16 pixel tile per block.
//            Phase one: every thread decodes its own texel (clamped into the image, so the threads of a partial tile fill the halo their
//            neighbours read), keeps the colour in registers and stores its luma into an 18 x 18 LDS tile; threads 0 .. 67 decode the 68
//            texels of the halo ring.  Each texel is decoded and square-rooted once per block, not once per tap.  A pixel whose luma range
//            is under the threshold stores its centre colour and is done.
//            Phase two: the pixels that search are appended to a per-block LDS list (ballot and prefix inside a wave, four wave counts
//            through LDS, no atomics) and the block's threads take the list's entries in order, so the waves that run the data-dependent
//            search loop are full but the last.  An entry is the pixel's index in the tile: the searching thread reads the nine lumas of
//            that pixel from the LDS tile and derives everything else from them.
//
// The search's samples are the manual clamp-mode bilinear of the oxc_apply_bloom block on the W x H source, four global loads each.  Every
// float operation keeps the order and rounding the header states: the file is compiled without contraction, division and sqrt are the
// IEEE ones.  The wave's FP16 denormal mode stays at its default (RGBA16F holds denormal halves).
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr int kHalo = 18;  // the side of the luma tile: 16 pixels and one texel of halo on each side

// rgb2luma (fxaa.slang:19)
OXC_DEV float luma_of(const V3& c) { return __builtin_sqrtf((c.x * 0.299f + c.y * 0.587f) + c.z * 0.114f); }

// QUALITY(q) (fxaa.slang:15)
OXC_DEV float quality(int q) { return q < 5 ? 1.0f : q > 5 ? (q < 10 ? 2.0f : q < 11 ? 4.0f : 8.0f) : 1.5f; }

template <int FORMAT>
OXC_DEV void store_rgba(void* base, size_t i, const Texel& t) {
  if (FORMAT == 0)
    static_cast<uint32_t*>(base)[i] = pack_ufloat<6>(t.c.x) | (pack_ufloat<6>(t.c.y) << 11) | (pack_ufloat<5>(t.c.z) << 22);
  else
    static_cast<uint2*>(base)[i] = make_uint2(channel_half(t.c.x) | (channel_half(t.c.y) << 16), channel_half(t.c.z) | (channel_half(t.a) << 16));
}

// Sample(sampler, uv) of the W x H source: the manual bilinear, clamp mode; the alpha only where the caller stores it
template <int FORMAT, bool ALPHA>
OXC_DEV Texel sample(const FxaaArgs& a, float u, float v) {
  const Axis ax = axis_at<false>(u, (float)a.w, (int)a.w - 1), ay = axis_at<false>(v, (float)a.h, (int)a.h - 1);
  const size_t r0 = (size_t)ay.i0 * a.w, r1 = (size_t)ay.i1 * a.w;
  const Texel t00 = load_rgba<FORMAT>(a.src, r0 + ax.i0), t10 = load_rgba<FORMAT>(a.src, r0 + ax.i1);
  const Texel t01 = load_rgba<FORMAT>(a.src, r1 + ax.i0), t11 = load_rgba<FORMAT>(a.src, r1 + ax.i1);
  Texel o;
  o.c = lerp3(lerp3(t00.c, t10.c, ax.f), lerp3(t01.c, t11.c, ax.f), ay.f);
  o.a = ALPHA && FORMAT == 1 ? lerp_f(lerp_f(t00.a, t10.a, ax.f), lerp_f(t01.a, t11.a, ax.f), ay.f) : 1.0f;
  return o;
}

// fxaa.slang:47-211 for pixel (x, y), whose luma sits at `c` in the LDS tile (its neighbours at +-1 and +-kHalo): the edge's orientation,
// the search along it and the final sample.  The statements keep the Slang's order.
template <int FORMAT, bool STATS>
OXC_DEV void search_pixel(const FxaaArgs& a, const float* c, uint32_t x, uint32_t y) {
  const float fw = (float)a.w, fh = (float)a.h;
  const float tex_x = ((float)x + 0.5f) / fw, tex_y = ((float)y + 0.5f) / fh;
  const float inv_x = 1.0f / fw, inv_y = 1.0f / fh;
  const float luma_center = c[0], luma_down = c[-kHalo], luma_up = c[kHalo], luma_left = c[-1], luma_right = c[1];
  const float luma_min = fminf(luma_center, fminf(fminf(luma_down, luma_up), fminf(luma_left, luma_right)));
  const float luma_max = fmaxf(luma_center, fmaxf(fmaxf(luma_down, luma_up), fmaxf(luma_left, luma_right)));
  const float luma_range = luma_max - luma_min;
  const float luma_down_left = c[-kHalo - 1], luma_up_right = c[kHalo + 1], luma_up_left = c[kHalo - 1], luma_down_right = c[-kHalo + 1];

  const float luma_down_up = luma_down + luma_up, luma_left_right = luma_left + luma_right;
  const float luma_left_corners = luma_down_left + luma_up_left, luma_down_corners = luma_down_left + luma_down_right;
  const float luma_right_corners = luma_down_right + luma_up_right, luma_up_corners = luma_up_right + luma_up_left;
  const float edge_horizontal = (__builtin_fabsf(-2.0f * luma_left + luma_left_corners) + __builtin_fabsf(-2.0f * luma_center + luma_down_up) * 2.0f) +
                                __builtin_fabsf(-2.0f * luma_right + luma_right_corners);
  const float edge_vertical = (__builtin_fabsf(-2.0f * luma_up + luma_up_corners) + __builtin_fabsf(-2.0f * luma_center + luma_left_right) * 2.0f) +
                              __builtin_fabsf(-2.0f * luma_down + luma_down_corners);
  const bool is_horizontal = edge_horizontal >= edge_vertical;
  float step_length = is_horizontal ? inv_y : inv_x;
  const float luma1 = is_horizontal ? luma_down : luma_left, luma2 = is_horizontal ? luma_up : luma_right;
  const float gradient1 = luma1 - luma_center, gradient2 = luma2 - luma_center;
  const bool is1_steepest = __builtin_fabsf(gradient1) >= __builtin_fabsf(gradient2);
  const float gradient_scaled = 0.25f * fmaxf(__builtin_fabsf(gradient1), __builtin_fabsf(gradient2));
  float luma_local_average;
  if (is1_steepest) {
    step_length = -step_length;
    luma_local_average = 0.5f * (luma1 + luma_center);
  } else {
    luma_local_average = 0.5f * (luma2 + luma_center);
  }
  float current_x = tex_x, current_y = tex_y;
  if (is_horizontal)
    current_y += step_length * 0.5f;
  else
    current_x += step_length * 0.5f;
  const float offset_x = is_horizontal ? inv_x : 0.0f, offset_y = is_horizontal ? 0.0f : inv_y;
  float uv1_x = current_x - offset_x * quality(0), uv1_y = current_y - offset_y * quality(0);
  float uv2_x = current_x + offset_x * quality(0), uv2_y = current_y + offset_y * quality(0);

  float luma_end1 = luma_of(sample<FORMAT, false>(a, uv1_x, uv1_y).c) - luma_local_average;
  float luma_end2 = luma_of(sample<FORMAT, false>(a, uv2_x, uv2_y).c) - luma_local_average;
  bool reached1 = __builtin_fabsf(luma_end1) >= gradient_scaled, reached2 = __builtin_fabsf(luma_end2) >= gradient_scaled;
  bool reached_both = reached1 && reached2;
  uint32_t taps = 2u;
  if (!reached1) uv1_x -= offset_x * quality(1), uv1_y -= offset_y * quality(1);
  if (!reached2) uv2_x += offset_x * quality(1), uv2_y += offset_y * quality(1);
  if (!reached_both) {
#pragma unroll 1
    for (int i = 2; i < 12; i++) {
      if (!reached1) luma_end1 = luma_of(sample<FORMAT, false>(a, uv1_x, uv1_y).c) - luma_local_average;
      if (!reached2) luma_end2 = luma_of(sample<FORMAT, false>(a, uv2_x, uv2_y).c) - luma_local_average;
      if (STATS) taps += (reached1 ? 0u : 1u) + (reached2 ? 0u : 1u);
      reached1 = __builtin_fabsf(luma_end1) >= gradient_scaled;
      reached2 = __builtin_fabsf(luma_end2) >= gradient_scaled;
      reached_both = reached1 && reached2;
      const float q = quality(i);
      if (!reached1) uv1_x -= offset_x * q, uv1_y -= offset_y * q;
      if (!reached2) uv2_x += offset_x * q, uv2_y += offset_y * q;
      if (reached_both) break;
    }
  }
  if (STATS) {
    atomicAdd(&a.stats[1], 1u);
    atomicAdd(&a.stats[2], taps);
    if (!reached_both) atomicAdd(&a.stats[3], 1u);
  }

  const float distance1 = is_horizontal ? tex_x - uv1_x : tex_y - uv1_y;
  const float distance2 = is_horizontal ? uv2_x - tex_x : uv2_y - tex_y;
  const bool is_direction1 = distance1 < distance2;
  const float distance_final = fminf(distance1, distance2);
  const float edge_thickness = distance1 + distance2;
  const bool is_luma_center_smaller = luma_center < luma_local_average;
  const bool correct_variation1 = (luma_end1 < 0.0f) != is_luma_center_smaller, correct_variation2 = (luma_end2 < 0.0f) != is_luma_center_smaller;
  const bool correct_variation = is_direction1 ? correct_variation1 : correct_variation2;
  const float pixel_offset = -distance_final / edge_thickness + 0.5f;
  float final_offset = correct_variation ? pixel_offset : 0.0f;

  const float luma_average = (1.0f / 12.0f) * ((2.0f * (luma_down_up + luma_left_right) + luma_left_corners) + luma_right_corners);
  const float sub_pixel_offset1 = fminf(fmaxf(__builtin_fabsf(luma_average - luma_center) / luma_range, 0.0f), 1.0f);
  const float sub_pixel_offset2 = ((-2.0f * sub_pixel_offset1 + 3.0f) * sub_pixel_offset1) * sub_pixel_offset1;
  const float sub_pixel_offset_final = (sub_pixel_offset2 * sub_pixel_offset2) * 0.75f;
  final_offset = fmaxf(final_offset, sub_pixel_offset_final);

  float final_x = tex_x, final_y = tex_y;
  if (is_horizontal)
    final_y += final_offset * step_length;
  else
    final_x += final_offset * step_length;
  store_rgba<FORMAT>(a.dst, (size_t)y * a.w + x, sample<FORMAT, true>(a, final_x, final_y));
}
}  // namespace

template <int FORMAT, bool STATS>
__global__ __launch_bounds__(256) void k_fxaa(FxaaArgs a) {
  __shared__ float luma[kHalo * kHalo];
  __shared__ uint8_t list[256];
  __shared__ uint32_t wave_count[4];
  const uint2 tp = tile_pixel();
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t lx = (wave & 1u) * 8u + (lane & 7u), ly = (wave >> 1) * 8u + (lane >> 3);  // the pixel's place in the tile, as tile_pixel()
  const int last_x = (int)a.w - 1, last_y = (int)a.h - 1;

  // phase one: the lumas of the tile and its halo, clamp addressing
  const Texel center = load_rgba<FORMAT>(a.src, (size_t)min(tp.y, a.h - 1u) * a.w + min(tp.x, a.w - 1u));
  luma[(ly + 1u) * kHalo + lx + 1u] = luma_of(center.c);
  if (tid < 68u) {  // the ring: the rows 0 and 17, then the columns 0 and 17 of the rows 1 .. 16
    const int hx = tid < 18u ? (int)tid : tid < 36u ? (int)tid - 18 : tid < 52u ? 0 : 17;
    const int hy = tid < 18u ? 0 : tid < 36u ? 17 : tid < 52u ? (int)tid - 35 : (int)tid - 51;
    const int gx = clamp_i((int)(blockIdx.x * 16u) + hx - 1, 0, last_x), gy = clamp_i((int)(blockIdx.y * 16u) + hy - 1, 0, last_y);
    luma[hy * kHalo + hx] = luma_of(load_rgba<FORMAT>(a.src, (size_t)gy * a.w + gx).c);
  }
  __syncthreads();

  bool searches = false;
  if (tp.x < a.w && tp.y < a.h) {
    const float* c = &luma[(ly + 1u) * kHalo + lx + 1u];
    const float luma_center = c[0], luma_down = c[-kHalo], luma_up = c[kHalo], luma_left = c[-1], luma_right = c[1];
    const float luma_min = fminf(luma_center, fminf(fminf(luma_down, luma_up), fminf(luma_left, luma_right)));
    const float luma_max = fmaxf(luma_center, fmaxf(fmaxf(luma_down, luma_up), fmaxf(luma_left, luma_right)));
    const float luma_range = luma_max - luma_min;
    if (luma_range < fmaxf(0.0312f, luma_max * 0.125f)) {
      store_rgba<FORMAT>(a.dst, (size_t)tp.y * a.w + tp.x, center);
      if (STATS) atomicAdd(&a.stats[0], 1u);
    } else {
      searches = true;
    }
  }

  // phase two: the searching pixels, compacted over the block
  const unsigned long long ballot = __ballot(searches);
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
  if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  uint32_t base = 0, total = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    const uint32_t n = wave_count[k];
    base += k < wave ? n : 0u;
    total += n;
  }
  if (searches) list[base + rank] = (uint8_t)(ly * 16u + lx);
  __syncthreads();
  if (tid < total) {  // at most 256 entries: one per thread, the waves full in order
    const uint32_t e = list[tid], ex = e & 15u, ey = e >> 4;
    search_pixel<FORMAT, STATS>(a, &luma[(ey + 1u) * kHalo + ex + 1u], blockIdx.x * 16u + ex, blockIdx.y * 16u + ey);
  }
}

void launch_fxaa(const FxaaArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  if (a.stats) {
    if (a.format == 0u)
      hipLaunchKernelGGL((k_fxaa<0, true>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((k_fxaa<1, true>), grid, dim3(256), 0, s, a);
  } else {
    if (a.format == 0u)
      hipLaunchKernelGGL((k_fxaa<0, false>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((k_fxaa<1, false>), grid, dim3(256), 0, s, a);
  }
}

}  // namespace oxc
