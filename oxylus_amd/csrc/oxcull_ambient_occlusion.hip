// oxcull_ambient_occlusion.hip -- VBGTAO ambient occlusion (gfx950): RendererInstance::generate_ambient_occlusion (Oxylus/src/Render/Passes/
// PBR.cpp:179-311; passes/gtao/vbgtao_prefilter.slang, vbgtao_main.slang, vbgtao_denoise.slang) as three compute launches.  Rules:
// include/oxcull.h, oxc_generate_ambient_occlusion; design and measurements: DESIGN.md section 14.
//
//   k_ao_prefilter   one wave per 16 x 16 source tile (four per block): a lane linearises its 2 x 2 texels (mip 0), averages them (mip 1) and
//                    the 8 x 8 mip-1 values of the wave are folded to mips 2..4 through cross-lane moves -- no LDS, no barrier.  Every lane
//                    works from its clamped gather whether or not its destination texels exist; only the stores are conditional.
//   k_ao_main        one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block), as k_vsm_resolve_shadow.  Settings and
//                    camera are kernel arguments (scalar loads); everything uniform per call is worked out once on the host.  A sky pixel
//                    is the five edge taps and two stores.  The slice and sample loops are uniform across the wave; the sixteen texels of
//                    a sample pair (2 sides x 2 levels x 4) are loaded unconditionally at clamped coordinates, in one batch.
//   k_ao_denoise     one thread per pixel: the 3 x 3 neighbourhood of the noisy image, the five packed edge words, the pow rule.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and square
// root are the IEEE ones, log2 / pow / the rotation pair are evaluated in binary64.  The wave's FP16 denormal mode stays at its default
// (denormals kept): no kernel here may call set_half_denorm_flush().
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr float kHalfPi = 1.57079632679f, kPi = 3.1415926535897932384626433832795f;

OXC_DEV float fast_acos(float in) {
  const float x = __builtin_fabsf(in);
  float res = -0.156583f * x + kHalfPi;
  res = res * __builtin_sqrtf(saturate_f(1.0f - x));
  return in >= 0.0f ? res : kPi - res;
}

OXC_DEV float unorm(uint32_t w, int k) { return (float)((w >> (8 * k)) & 0xFFu) / 255.0f; }

OXC_DEV float weighted_average(float d0, float d1, float d2, float d3, float mul, float add) {
  const float mn = fminf(fminf(d0, d1), fminf(d2, d3));
  const float w0 = saturate_f((d0 - mn) * mul + add), w1 = saturate_f((d1 - mn) * mul + add);
  const float w2 = saturate_f((d2 - mn) * mul + add), w3 = saturate_f((d3 - mn) * mul + add);
  const float total = ((w0 + w1) + w2) + w3;
  return ((((w0 * d0) + (w1 * d1)) + (w2 * d2)) + (w3 * d3)) / total;
}

struct Tap {
  const float *r0, *r1;  // the two texel rows
  uint32_t x0, x1;
  float fx, fy;
};
// the manual bilinear's addresses and fractions at one level (rule: as oxc_contact_shadows step 6).  The level's extent is max(1, dim >> level)
// and its offset a select chain: an index into the argument block that differs per lane would go through scratch.
OXC_DEV Tap tap_of(const AmbientOcclusionArgs& a, int level, float u, float v) {
  const uint32_t w = max(a.w >> level, 1u), h = max(a.h >> level, 1u);
  const uint64_t off = level == 0 ? a.lvl_off[0] : level == 1 ? a.lvl_off[1] : level == 2 ? a.lvl_off[2] : level == 3 ? a.lvl_off[3] : a.lvl_off[4];
  const int wm1 = (int)w - 1, hm1 = (int)h - 1;
  const float gx = u * (float)w - 0.5f, gy = v * (float)h - 0.5f;
  const float ix = floorf(gx), iy = floorf(gy);
  Tap t;
  t.fx = gx - ix;
  t.fy = gy - iy;
  const int bx = clamp_i(cvt_i32_sat(ix), -1, wm1), by = clamp_i(cvt_i32_sat(iy), -1, hm1);  // i + 1 cannot wrap after this
  t.x0 = (uint32_t)max(bx, 0);
  t.x1 = (uint32_t)min(bx + 1, wm1);
  t.r0 = a.pre + off + (uint64_t)((uint32_t)max(by, 0) * w);
  t.r1 = a.pre + off + (uint64_t)((uint32_t)min(by + 1, hm1) * w);
  return t;
}
OXC_DEV float bil(const Tap& t, float t00, float t10, float t01, float t11) {
  const float top = t00 + (t10 - t00) * t.fx, bot = t01 + (t11 - t01) * t.fx;
  return top + (bot - top) * t.fy;
}

OXC_DEV float dotv(const V3& a, const V3& b) { return dot3(a.x, a.y, a.z, b.x, b.y, b.z); }

// update_sectors into an empty bitmask; zero: the arc has no width
OXC_DEV uint32_t update_sectors(float min_h, float max_h, bool& zero) {
  const uint32_t angle = cvt_u32_sat(ceilf(saturate_f(max_h - min_h) * 32.0f));
  zero = angle == 0u;
  const uint32_t start = min(cvt_u32_sat(saturate_f(min_h) * 32.0f), 31u);
  const uint32_t bits = 0xFFFFFFFFu >> (32u - max(angle, 1u));
  return zero ? 0u : bits << start;
}

template <bool STATS>
OXC_DEV uint32_t sector_mask(float thickness, const V3& delta, const V3& vd, float side, float n, uint32_t* st) {
  const V3 back = {delta.x - vd.x * thickness, delta.y - vd.y * thickness, delta.z - vd.z * thickness};
  float hf = fast_acos(dotv(normalize3(delta), vd));
  float hb = fast_acos(dotv(normalize3(back), vd));
  hf = saturate_f((((side * -hf) + n) + kHalfPi) / kPi);
  hb = saturate_f((((side * -hb) + n) + kHalfPi) / kPi);
  bool zero;
  const uint32_t m = side >= 0.0f ? update_sectors(hb, hf, zero) : update_sectors(hf, hb, zero);
  if (STATS && zero) st[11]++;
  return m;
}
}  // namespace

__global__ __launch_bounds__(256) void k_ao_prefilter(AmbientOcclusionArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t bx = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t by = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
  // (a wave whose tile lies outside the image has no destination texel at any level: its first source texel is at >= extent)
  if ((blockIdx.x * 16u + (wave & 1u) * 8u) * 2u >= a.w || (blockIdx.y * 16u + (wave >> 1) * 8u) * 2u >= a.h) return;
  const uint32_t x0 = min(2u * bx, a.w - 1u), x1 = min(2u * bx + 1u, a.w - 1u), y0 = min(2u * by, a.h - 1u), y1 = min(2u * by + 1u, a.h - 1u);
  const float* r0 = a.depth + (size_t)y0 * a.w;
  const float* r1 = a.depth + (size_t)y1 * a.w;
  const float s00 = r0[x0], s10 = r0[x1], s01 = r1[x0], s11 = r1[x1];
  const float d00 = a.lin_mul / (s00 + a.lin_add), d10 = a.lin_mul / (s10 + a.lin_add);
  const float d01 = a.lin_mul / (s01 + a.lin_add), d11 = a.lin_mul / (s11 + a.lin_add);
  const bool inx0 = 2u * bx < a.w, inx1 = 2u * bx + 1u < a.w, iny0 = 2u * by < a.h, iny1 = 2u * by + 1u < a.h;
  float* l0 = a.pre + a.lvl_off[0];
  if (inx0 && iny0) l0[(size_t)(2u * by) * a.w + 2u * bx] = d00;
  if (inx1 && iny0) l0[(size_t)(2u * by) * a.w + 2u * bx + 1u] = d10;
  if (inx0 && iny1) l0[(size_t)(2u * by + 1u) * a.w + 2u * bx] = d01;
  if (inx1 && iny1) l0[(size_t)(2u * by + 1u) * a.w + 2u * bx + 1u] = d11;
  float m = weighted_average(d00, d10, d01, d11, a.pf_mul, a.pf_add);
  if (bx < a.lvl_w[1] && by < a.lvl_h[1]) a.pre[a.lvl_off[1] + (uint64_t)(by * a.lvl_w[1] + bx)] = m;
#pragma unroll
  for (uint32_t k = 2; k < 5; k++) {
    const uint32_t step = 1u << (k - 2u);  // lanes `step` apart hold neighbouring values of level k - 1
    const float n1 = bperm_f((int)(lane + step), m), n2 = bperm_f((int)(lane + 8u * step), m), n3 = bperm_f((int)(lane + 9u * step), m);
    m = weighted_average(m, n1, n2, n3, a.pf_mul, a.pf_add);  // meaningful in the lanes whose x and y are multiples of 2 * step
    const uint32_t mask = 2u * step - 1u;
    const uint32_t dx = bx >> (k - 1u), dy = by >> (k - 1u);
    if (!(lane & mask) && !((lane >> 3) & mask) && dx < a.lvl_w[k] && dy < a.lvl_h[k]) a.pre[a.lvl_off[k] + (uint64_t)(dy * a.lvl_w[k] + dx)] = m;
  }
}

template <bool STATS>
__global__ __launch_bounds__(256) void k_ao_main(AmbientOcclusionArgs a) {
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const size_t pix = (size_t)py * a.w + px;
  const float* pre = a.pre;

  // calculate_edges: the five texels of level 0, clamped
  float centre;
  {
    const uint32_t xl = max(px, 1u) - 1u, xr = min(px + 1u, a.w - 1u), yt = max(py, 1u) - 1u, yb = min(py + 1u, a.h - 1u);
    const float* l0 = pre + a.lvl_off[0];
    centre = l0[pix];
    const float left = l0[(size_t)py * a.w + xl], right = l0[(size_t)py * a.w + xr], top = l0[(size_t)yt * a.w + px], bottom = l0[(size_t)yb * a.w + px];
    const float e0 = left - centre, e1 = right - centre, e2 = top - centre, e3 = bottom - centre;
    const float slr = (e1 - e0) * 0.5f, stb = (e3 - e2) * 0.5f;
    const float scale = centre * 0.011f;
    const float bias = 1.0f + 0.25f;
    const float q0 = bias - fminf(__builtin_fabsf(e0), __builtin_fabsf(e0 + slr)) / scale;
    const float q1 = bias - fminf(__builtin_fabsf(e1), __builtin_fabsf(e1 + -slr)) / scale;
    const float q2 = bias - fminf(__builtin_fabsf(e2), __builtin_fabsf(e2 + stb)) / scale;
    const float q3 = bias - fminf(__builtin_fabsf(e3), __builtin_fabsf(e3 + -stb)) / scale;
    a.edges[pix] = pack_unorm(q0) | (pack_unorm(q1) << 8) | (pack_unorm(q2) << 16) | (pack_unorm(q3) << 24);
  }
  if (centre >= a.far_thr) {  // sky (a NaN depth is not)
    a.noisy[pix] = 0x3C00u;
    return;
  }
  // STATS: {non-sky, samples, mip 0..4, fractional, == 1.0, inside (0, 1), == 0.0, zero width, sign -1, 0, +1}
  uint32_t st[15] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};

  const float uvx = ((float)px + 0.5f) / a.res_x, uvy = ((float)py + 0.5f) / a.res_y;
  const float ld = centre * 0.99999f;
  const V3 origin = {((uvx * 2.0f - 1.0f) / a.p00) * ld, ((uvy * 2.0f - 1.0f) / a.p11) * ld, -ld};
  const V3 vd = normalize3({-origin.x, -origin.y, -origin.z});

  // load_normal_view_space: the texel at the pixel
  V3 nrm;
  {
    const V3 wn = normalize3(oct_normal_ba(a.normal[pix * 2u + 1u]));
    nrm = normalize3({(a.view3[0] * wn.x + a.view3[1] * wn.y) + a.view3[2] * wn.z, (a.view3[3] * wn.x + a.view3[4] * wn.y) + a.view3[5] * wn.z,
                      (a.view3[6] * wn.x + a.view3[7] * wn.y) + a.view3[8] * wn.z});
  }
  // load_noise
  const float idx = (float)((uint32_t)a.hilbert[(py & 63u) * 64u + (px & 63u)] + a.noise_add);
  const float t0 = 0.5f + idx * 0.75487766624669276005f, t1 = 0.5f + idx * 0.5698402909980532659114f;
  const float noise_x = t0 - floorf(t0), noise_y = t1 - floorf(t1);

  const float srx = a.radius_x / ld, sry = a.radius_y / ld;
  const float min_s = 1.3f / fmaxf(srx * a.res_x, 1.3f);

  float visibility = 0.0f;
#pragma unroll 1
  for (uint32_t si = 0; si < a.slice_count; si++) {
    const float slice_t = (float)si;
    const float slice = (slice_t + noise_x) / a.slice_count_f;
    float c, s;
    cos_sin_turn(slice * 0.5f, c, s);
    const float dv = c * vd.x + s * vd.y;
    const V3 ortho = normalize3({c - dv * vd.x, s - dv * vd.y, 0.0f - dv * vd.z});
    const V3 axis = normalize3({s * vd.z, -(c * vd.z), c * vd.y - s * vd.x});
    const float na = dotv(nrm, axis);
    const V3 pn = {nrm.x - axis.x * na, nrm.y - axis.y * na, nrm.z - axis.z * na};
    const float pnl = fmaxf(len3(pn.x, pn.y, pn.z), 1e-6f);
    const float sg = sign_f(dotv(ortho, pn));
    const float n = sg * fast_acos(saturate_f(dotv(pn, vd) / pnl));
    if (STATS) {
      st[12] += sg < 0.0f ? 1u : 0u;
      st[13] += sg == 0.0f ? 1u : 0u;
      st[14] += sg > 0.0f ? 1u : 0u;
    }
    const float smx = c * srx, smy = (-s) * sry;

    uint32_t bitmask = 0u;
    float occlusion = 0.0f;
#pragma unroll 1
    for (uint32_t ti = 0; ti < a.samples; ti++) {
      const float sample_t = (float)ti;
      const float u0 = noise_y + (slice_t + sample_t * a.samples_f) * 0.6180339887498948482f;
      const float sn = u0 - floorf(u0);
      float sv = (sample_t + sn) / a.samples_f;
      sv = sv * sv;
      sv = sv + min_s;
      const float ox = sv * smx, oy = sv * smy;
      const float u1 = uvx + ox, v1 = uvy + oy, u2 = uvx - ox, v2 = uvy - oy;
      const float lx = ox * a.res_x, ly = oy * a.res_y;
      const float lvl = fminf(fmaxf((float)log2_f64(__builtin_sqrtf(lx * lx + ly * ly)) - 3.30f, 0.0f), 4.0f);
      const float lfl = floorf(lvl), lfr = lvl - lfl;
      const int l0 = (int)lfl, l1 = min(l0 + 1, 4);
      // sixteen texels, one batch
      const Tap a1 = tap_of(a, l0, u1, v1), b1 = tap_of(a, l1, u1, v1), a2 = tap_of(a, l0, u2, v2), b2 = tap_of(a, l1, u2, v2);
      const float a1_00 = a1.r0[a1.x0], a1_10 = a1.r0[a1.x1], a1_01 = a1.r1[a1.x0], a1_11 = a1.r1[a1.x1];
      const float b1_00 = b1.r0[b1.x0], b1_10 = b1.r0[b1.x1], b1_01 = b1.r1[b1.x0], b1_11 = b1.r1[b1.x1];
      const float a2_00 = a2.r0[a2.x0], a2_10 = a2.r0[a2.x1], a2_01 = a2.r1[a2.x0], a2_11 = a2.r1[a2.x1];
      const float b2_00 = b2.r0[b2.x0], b2_10 = b2.r0[b2.x1], b2_01 = b2.r1[b2.x0], b2_11 = b2.r1[b2.x1];
      const float da1 = bil(a1, a1_00, a1_10, a1_01, a1_11), db1 = bil(b1, b1_00, b1_10, b1_01, b1_11);
      const float da2 = bil(a2, a2_00, a2_10, a2_01, a2_11), db2 = bil(b2, b2_00, b2_10, b2_01, b2_11);
      const float d1 = da1 + (db1 - da1) * lfr, d2 = da2 + (db2 - da2) * lfr;
      if (STATS) {
        st[1] += 2u;
#pragma unroll
        for (int k = 0; k < 5; k++) st[2 + k] += l0 == k ? 2u : 0u;
        if (lfr != 0.0f) st[7] += 2u;
      }
      const V3 delta1 = {((u1 * 2.0f - 1.0f) / a.p00) * d1 - origin.x, ((v1 * 2.0f - 1.0f) / a.p11) * d1 - origin.y, -d1 - origin.z};
      const V3 delta2 = {((u2 * 2.0f - 1.0f) / a.p00) * d2 - origin.x, ((v2 * 2.0f - 1.0f) / a.p11) * d2 - origin.y, -d2 - origin.z};
      const uint32_t m1 = sector_mask<STATS>(a.thickness, delta1, vd, 1.0f, n, st);
      const uint32_t m2 = sector_mask<STATS>(a.thickness, delta2, vd, -1.0f, n, st);
      const float f1 = saturate_f(len3(delta1.x, delta1.y, delta1.z) * a.falloff_mul + a.falloff_add);
      const float f2_ = saturate_f(len3(delta2.x, delta2.y, delta2.z) * a.falloff_mul + a.falloff_add);
      occlusion = occlusion + (f1 * (float)__builtin_popcount(m1 & ~bitmask)) / 32.0f;
      bitmask |= m1;
      occlusion = occlusion + (f2_ * (float)__builtin_popcount(m2 & ~bitmask)) / 32.0f;
      bitmask |= m2;
    }
    visibility = visibility + saturate_f(1.0f - occlusion);
  }
  const unsigned short hv = f_to_half(saturate_f(visibility / a.slice_count_f));
  a.noisy[pix] = hv;
  if (STATS) {
    st[8] += hv == 0x3C00u ? 1u : 0u;
    st[10] += hv == 0u ? 1u : 0u;
    st[9] += hv != 0x3C00u && hv != 0u ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < 15; k++)
      if (st[k]) atomicAdd(&a.stats[k], st[k]);
  }
}

__global__ __launch_bounds__(256) void k_ao_denoise(AmbientOcclusionArgs a) {
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const uint32_t xl = max(px, 1u) - 1u, xr = min(px + 1u, a.w - 1u), yt = max(py, 1u) - 1u, yb = min(py + 1u, a.h - 1u);
  const size_t rt = (size_t)yt * a.w, rc = (size_t)py * a.w, rb = (size_t)yb * a.w;
  // fourteen loads, one batch
  const uint32_t ec = a.edges[rc + px], el = a.edges[rc + xl], er = a.edges[rc + xr], et = a.edges[rt + px], eb = a.edges[rb + px];
  const float v_tl = dequantize_half(a.noisy[rt + xl]), v_t = dequantize_half(a.noisy[rt + px]), v_tr = dequantize_half(a.noisy[rt + xr]);
  const float v_l = dequantize_half(a.noisy[rc + xl]), v_c = dequantize_half(a.noisy[rc + px]), v_r = dequantize_half(a.noisy[rc + xr]);
  const float v_bl = dequantize_half(a.noisy[rb + xl]), v_b = dequantize_half(a.noisy[rb + px]), v_br = dequantize_half(a.noisy[rb + xr]);

  const float lw = unorm(ec, 0) * unorm(el, 1), rw = unorm(ec, 1) * unorm(er, 0), tw = unorm(ec, 2) * unorm(et, 3), bw = unorm(ec, 3) * unorm(eb, 2);
  const float tlw = 0.425f * (tw * unorm(et, 0) + lw * unorm(el, 2));
  const float trw = 0.425f * (tw * unorm(et, 1) + rw * unorm(er, 2));
  const float blw = 0.425f * (bw * unorm(eb, 0) + lw * unorm(el, 3));
  const float brw = 0.425f * (bw * unorm(eb, 1) + rw * unorm(er, 3));
  const float cw = 1.2f;
  float sum = v_c * cw;
  sum = sum + v_l * lw;
  sum = sum + v_r * rw;
  sum = sum + v_t * tw;
  sum = sum + v_b * bw;
  sum = sum + v_tl * tlw;
  sum = sum + v_tr * trw;
  sum = sum + v_bl * blw;
  sum = sum + v_br * brw;
  float sw = cw;
  sw = sw + lw;
  sw = sw + rw;
  sw = sw + tw;
  sw = sw + bw;
  sw = sw + tlw;
  sw = sw + trw;
  sw = sw + blw;
  sw = sw + brw;
  a.out[rc + px] = f_to_half(pow_rule(fmaxf(sum / sw, 0.0f), a.final_power));
}

void launch_ambient_occlusion(const AmbientOcclusionArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  hipLaunchKernelGGL(k_ao_prefilter, dim3((a.w + 31u) / 32u, (a.h + 31u) / 32u), dim3(256), 0, s, a);
  if (a.stats)
    hipLaunchKernelGGL(k_ao_main<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_ao_main<false>, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ao_denoise, grid, dim3(256), 0, s, a);
}

}  // namespace oxc
