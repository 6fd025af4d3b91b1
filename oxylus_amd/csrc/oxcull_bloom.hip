// oxcull_bloom.hip -- the bloom prefilter and its two mip pyramids (gfx950): RendererInstance::apply_bloom
// (Oxylus/src/Render/Passes/PostProcess.cpp:79-203, passes/bloom_prefilter.slang, passes/bloom_downsample.slang and
// passes/bloom_upsample.slang).  Rules: include/oxcull.h, oxc_apply_bloom; design and measurements: DESIGN.md section 18.
//
//   k_bloom_prefilter   16 x 16 output pixels per block over D level 0: 13 border taps of the W x H source, the five groups, the
//                 thresholded and luminance-weighted average.  Thread 0 of block (0, 0) also stores the one texel of U level L - 1 (the
//                 clear of step 1): a store in a kernel, because a captured memset node does not replay, and no
//                 launch of its own, because nothing reads that texel.
//   k_bloom_downsample  one launch per level k: 13 border taps of D level k - 1.
//   k_bloom_upsample    one launch per level k: 9 clamped taps of U level k (D level L - 1 for the first), one load of D level k - 1.
//   k_bloom_tail        one block of 256 threads runs the downsample levels T .. L - 1 and the upsample levels L - 1 .. T in one launch,
//                 every thread taking the pixels tid, tid + 256, ... of a level.  A level reads texels the same block stored in the level
//                 before: __syncthreads() between the levels orders those global stores before the loads (the block's waves share one CU
//                 and its vector cache; no load of such a texel is issued before the barrier).  The levels it runs are a few hundred texels:
//                 as launches of their own they cost a launch each and fill a fraction of one CU.
//
// A tap's coordinates are the rule's binary32 arithmetic, per axis: the column and its weight depend on x alone, the row and its weight on
// y alone, so a pixel computes five of each (offsets -2 .. 2) and every tap picks a pair.  Every float operation keeps the order and
// rounding the header states: the file is compiled without contraction and division is the IEEE one.  The wave's FP16 denormal mode stays at
// its default (RGBA16F holds denormal halves).
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr uint32_t kTailTexels = 1024;  // the tail kernel starts at the first level whose source level has at most this many texels
constexpr uint32_t kTailTexelsForced = 16384;  // and a forced start is raised to the first level whose source level has at most this many

OXC_DEV V3 add3(const V3& a, const V3& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
OXC_DEV V3 mul3(const V3& a, float s) { return {a.x * s, a.y * s, a.z * s}; }
OXC_DEV V3 sum4(const V3& a, const V3& b, const V3& c, const V3& d) { return add3(add3(add3(a, b), c), d); }

OXC_DEV uint32_t level_side(uint32_t side, uint32_t k) { return max(1u, side >> k); }

template <int FORMAT>
OXC_DEV V3 load_texel(const void* base, size_t i) {
  if (FORMAT == 0) {
    const uint32_t w = static_cast<const uint32_t*>(base)[i];
    return {unpack_ufloat<6>(w & 0x7FFu), unpack_ufloat<6>((w >> 11) & 0x7FFu), unpack_ufloat<5>(w >> 22)};
  }
  const uint2 v = static_cast<const uint2*>(base)[i];
  return {dequantize_half(v.x & 0xFFFFu), dequantize_half(v.x >> 16), dequantize_half(v.y & 0xFFFFu)};
}

template <int FORMAT>
OXC_DEV void store_texel(void* base, size_t i, const V3& c) {
  if (FORMAT == 0)
    static_cast<uint32_t*>(base)[i] = pack_ufloat<6>(c.x) | (pack_ufloat<6>(c.y) << 11) | (pack_ufloat<5>(c.z) << 22);
  else
    static_cast<uint2*>(base)[i] = make_uint2(channel_half(c.x) | (channel_half(c.y) << 16), channel_half(c.z) | (0x3C00u << 16));
}

// uv = (f32(x) + 0.5) / f32(extent of the output), ts = 1.0 / that extent, k the tap offset, fsize / last the source level's side
template <bool BORDER>
OXC_DEV Axis axis_tap(float uv, float ts, float k, float fsize, int last) {
  return axis_at<BORDER>(uv + ts * k, fsize, last);
}

template <int FORMAT, bool BORDER>
OXC_DEV V3 tap(const void* src, uint32_t sw, const Axis& ax, const Axis& ay) {
  const V3 zero = {0.0f, 0.0f, 0.0f};
  const size_t r0 = (size_t)ay.i0 * sw, r1 = (size_t)ay.i1 * sw;
  const V3 t00 = !BORDER || (ax.in0 && ay.in0) ? load_texel<FORMAT>(src, r0 + ax.i0) : zero;
  const V3 t10 = !BORDER || (ax.in1 && ay.in0) ? load_texel<FORMAT>(src, r0 + ax.i1) : zero;
  const V3 t01 = !BORDER || (ax.in0 && ay.in1) ? load_texel<FORMAT>(src, r1 + ax.i0) : zero;
  const V3 t11 = !BORDER || (ax.in1 && ay.in1) ? load_texel<FORMAT>(src, r1 + ax.i1) : zero;
  return lerp3(lerp3(t00, t10, ax.f), lerp3(t01, t11, ax.f), ay.f);
}

// The axes of output pixel (x, y) of an ow x oh output reading an sw x sh level, for the offsets -R .. R
template <bool BORDER, int R>
struct Axes {
  Axis x[2 * R + 1], y[2 * R + 1];
  OXC_DEV Axes(uint32_t sw, uint32_t sh, uint32_t ow, uint32_t oh, uint32_t px, uint32_t py) {
    const float fow = (float)ow, foh = (float)oh;
    const float u = ((float)px + 0.5f) / fow, v = ((float)py + 0.5f) / foh;
    const float tx = 1.0f / fow, ty = 1.0f / foh;
#pragma unroll
    for (int k = -R; k <= R; k++) {
      x[k + R] = axis_tap<BORDER>(u, tx, (float)k, (float)sw, (int)sw - 1);
      y[k + R] = axis_tap<BORDER>(v, ty, (float)k, (float)sh, (int)sh - 1);
    }
  }
};

// the 13 taps of bloom_prefilter.slang:51-63 and bloom_downsample.slang:21-33, border
struct Taps13 {
  V3 a, b, c, d, e, f, g, h, i, j, k, l, m;
};

template <int FORMAT>
OXC_DEV Taps13 sample13(const void* src, uint32_t sw, uint32_t sh, uint32_t ow, uint32_t oh, uint32_t px, uint32_t py) {
  const Axes<true, 2> ax(sw, sh, ow, oh, px, py);
  auto at = [&](int kx, int ky) { return tap<FORMAT, true>(src, sw, ax.x[kx + 2], ax.y[ky + 2]); };
  Taps13 t;
  t.a = at(-2, 2), t.b = at(0, 2), t.c = at(2, 2);
  t.d = at(-2, 0), t.e = at(0, 0), t.f = at(2, 0);
  t.g = at(-2, -2), t.h = at(0, -2), t.i = at(2, -2);
  t.j = at(-1, 1), t.k = at(1, 1), t.l = at(-1, -1), t.m = at(1, -1);
  return t;
}

// step 2 for one group: clamp, weight, threshold curve, accumulate
OXC_DEV void accumulate_group(V3 g, float threshold, float soft_threshold, float clamp_value, V3& color_sum, float& weight_sum) {
  g = {fminf(g.x, clamp_value), fminf(g.y, clamp_value), fminf(g.z, clamp_value)};
  const float weight = 1.0f / (1.0f + ((g.x * 0.299f + g.y * 0.587f) + g.z * 0.114f));
  const float brightness = fmaxf(g.x, fmaxf(g.y, g.z));
  const float knee = threshold * soft_threshold;
  float soft = fminf(fmaxf((brightness - threshold) + knee, 0.0f), 2.0f * knee);
  soft = ((soft * soft) * 0.25f) / (knee + 1.0e-5f);
  const float contribution = fmaxf(soft, brightness - threshold) / fmaxf(brightness, 1.0e-5f);
  color_sum = add3(color_sum, mul3(mul3(g, contribution), weight));
  weight_sum += weight;
}

// step 3 for one pixel of D level k
template <int FORMAT>
OXC_DEV void downsample_pixel(const void* src, uint32_t sw, uint32_t sh, void* dst, uint32_t ow, uint32_t oh, uint32_t px, uint32_t py) {
  const Taps13 t = sample13<FORMAT>(src, sw, sh, ow, oh, px, py);
  const V3 corners = mul3(sum4(t.a, t.c, t.g, t.i), 0.03125f), edges = mul3(sum4(t.b, t.d, t.f, t.h), 0.0625f);
  const V3 inner = mul3(add3(sum4(t.e, t.j, t.k, t.l), t.m), 0.125f);
  store_texel<FORMAT>(dst, (size_t)py * ow + px, add3(add3(corners, edges), inner));
}

// step 4 for one pixel of U level k - 1: `src` the 9-tap source, `down` D level k - 1
template <int FORMAT>
OXC_DEV void upsample_pixel(const void* src, uint32_t sw, uint32_t sh, const void* down, void* dst, uint32_t ow, uint32_t oh, uint32_t px, uint32_t py,
                            float radius) {
  const Axes<false, 1> ax(sw, sh, ow, oh, px, py);
  auto at = [&](int kx, int ky) { return tap<FORMAT, false>(src, sw, ax.x[kx + 1], ax.y[ky + 1]); };
  const V3 a = at(-1, 1), b = at(0, 1), c = at(1, 1), d = at(-1, 0), e = at(0, 0), f = at(1, 0), g = at(-1, -1), h = at(0, -1), i = at(1, -1);
  const V3 color_sum = add3(add3(mul3(e, 0.25f), mul3(sum4(b, d, f, h), 0.125f)), mul3(sum4(a, c, g, i), 0.0625f));
  const size_t pix = (size_t)py * ow + px;
  store_texel<FORMAT>(dst, pix, lerp3(load_texel<FORMAT>(down, pix), color_sum, radius));
}
}  // namespace

template <int FORMAT>
__global__ __launch_bounds__(256) void k_bloom_prefilter(BloomArgs a) {
  if (blockIdx.x == 0u && blockIdx.y == 0u && threadIdx.x == 0u) store_texel<FORMAT>(a.up[a.levels - 1u], 0, V3{0.0f, 0.0f, 0.0f});  // step 1
  const uint2 tp = tile_pixel();
  if (tp.x >= a.w2 || tp.y >= a.h2) return;
  const Taps13 t = sample13<FORMAT>(a.src, a.w, a.h, a.w2, a.h2, tp.x, tp.y);
  const float exposure = a.exposure ? a.exposure[1] : 1.0f;
  V3 color_sum = {0.0f, 0.0f, 0.0f};
  float weight_sum = 0.0f;
  accumulate_group(mul3(mul3(sum4(t.a, t.b, t.d, t.e), 0.25f), exposure), a.threshold, a.soft_threshold, a.clamp_value, color_sum, weight_sum);
  accumulate_group(mul3(mul3(sum4(t.b, t.c, t.e, t.f), 0.25f), exposure), a.threshold, a.soft_threshold, a.clamp_value, color_sum, weight_sum);
  accumulate_group(mul3(mul3(sum4(t.d, t.e, t.g, t.h), 0.25f), exposure), a.threshold, a.soft_threshold, a.clamp_value, color_sum, weight_sum);
  accumulate_group(mul3(mul3(sum4(t.e, t.f, t.h, t.i), 0.25f), exposure), a.threshold, a.soft_threshold, a.clamp_value, color_sum, weight_sum);
  accumulate_group(mul3(mul3(sum4(t.j, t.k, t.l, t.m), 0.25f), exposure), a.threshold, a.soft_threshold, a.clamp_value, color_sum, weight_sum);
  const float denominator = weight_sum + 1.0e-5f;
  store_texel<FORMAT>(a.down[0], (size_t)tp.y * a.w2 + tp.x, V3{color_sum.x / denominator, color_sum.y / denominator, color_sum.z / denominator});
}

template <int FORMAT>
__global__ __launch_bounds__(256) void k_bloom_downsample(const void* src, uint32_t sw, uint32_t sh, void* dst, uint32_t ow, uint32_t oh) {
  const uint2 tp = tile_pixel();
  if (tp.x >= ow || tp.y >= oh) return;
  downsample_pixel<FORMAT>(src, sw, sh, dst, ow, oh, tp.x, tp.y);
}

template <int FORMAT>
__global__ __launch_bounds__(256) void k_bloom_upsample(const void* src, uint32_t sw, uint32_t sh, const void* down, void* dst, uint32_t ow, uint32_t oh,
                                                        float radius) {
  const uint2 tp = tile_pixel();
  if (tp.x >= ow || tp.y >= oh) return;
  upsample_pixel<FORMAT>(src, sw, sh, down, dst, ow, oh, tp.x, tp.y, radius);
}

// Levels a.tail .. L - 1 down and back in one block.  No pointer of it is __restrict__: a level's loads must not move above the barrier
// behind the stores of the level before.
template <int FORMAT>
__global__ __launch_bounds__(256) void k_bloom_tail(BloomArgs a) {
  const uint32_t tid = threadIdx.x, last = a.levels - 1u;
#pragma unroll 1
  for (uint32_t k = a.tail; k <= last; k++) {
    const uint32_t sw = level_side(a.w2, k - 1u), sh = level_side(a.h2, k - 1u), ow = level_side(a.w2, k), oh = level_side(a.h2, k);
#pragma unroll 1
    for (uint32_t p = tid; p < ow * oh; p += 256u) downsample_pixel<FORMAT>(a.down[k - 1u], sw, sh, a.down[k], ow, oh, p % ow, p / ow);
    __syncthreads();
  }
#pragma unroll 1
  for (uint32_t k = last; k >= a.tail; k--) {  // a.tail >= 1
    const uint32_t sw = level_side(a.w2, k), sh = level_side(a.h2, k), ow = level_side(a.w2, k - 1u), oh = level_side(a.h2, k - 1u);
    const void* const src = k == last ? a.down[last] : a.up[k];
#pragma unroll 1
    for (uint32_t p = tid; p < ow * oh; p += 256u) upsample_pixel<FORMAT>(src, sw, sh, a.down[k - 1u], a.up[k - 1u], ow, oh, p % ow, p / ow, a.radius);
    __syncthreads();
  }
}

// the first level whose source level has at most `texels` texels; L when there is none
static uint32_t first_tail_level(uint32_t w2, uint32_t h2, uint32_t levels, uint32_t texels) {
  for (uint32_t k = 1; k < levels; k++)
    if ((uint64_t)std::max(1u, w2 >> (k - 1u)) * std::max(1u, h2 >> (k - 1u)) <= texels) return k;
  return levels;
}
// T by default, and the lowest T the tuning id can force
uint32_t bloom_default_tail(uint32_t w2, uint32_t h2, uint32_t levels) { return first_tail_level(w2, h2, levels, kTailTexels); }
uint32_t bloom_lowest_tail(uint32_t w2, uint32_t h2, uint32_t levels) { return first_tail_level(w2, h2, levels, kTailTexelsForced); }

template <int FORMAT>
static void launch_bloom_format(const BloomArgs& a, hipStream_t s) {
  const auto grid = [](uint32_t w, uint32_t h) { return dim3((w + 15u) / 16u, (h + 15u) / 16u); };
  const auto side = [](uint32_t v, uint32_t k) { return std::max(1u, v >> k); };
  const uint32_t L = a.levels, T = a.tail;
  hipLaunchKernelGGL((k_bloom_prefilter<FORMAT>), grid(a.w2, a.h2), dim3(256), 0, s, a);
  for (uint32_t k = 1; k < T && k < L; k++)
    hipLaunchKernelGGL((k_bloom_downsample<FORMAT>), grid(side(a.w2, k), side(a.h2, k)), dim3(256), 0, s, (const void*)a.down[k - 1u], side(a.w2, k - 1u),
                       side(a.h2, k - 1u), a.down[k], side(a.w2, k), side(a.h2, k));
  if (T < L) hipLaunchKernelGGL((k_bloom_tail<FORMAT>), dim3(1), dim3(256), 0, s, a);
  for (uint32_t k = std::min(T, L) - 1u; k >= 1u; k--)
    hipLaunchKernelGGL((k_bloom_upsample<FORMAT>), grid(side(a.w2, k - 1u), side(a.h2, k - 1u)), dim3(256), 0, s,
                       (const void*)(k == L - 1u ? a.down[k] : a.up[k]), side(a.w2, k), side(a.h2, k), (const void*)a.down[k - 1u], a.up[k - 1u],
                       side(a.w2, k - 1u), side(a.h2, k - 1u), a.radius);
}

void launch_bloom(const BloomArgs& a, hipStream_t s) {
  if (a.format == 0u)
    launch_bloom_format<0>(a, s);
  else
    launch_bloom_format<1>(a, s);
}

}  // namespace oxc
