// oxcull_pixel_device.hpp -- the device rules the VSM page update and the per-pixel passes (visbuffer decode, shadow resolve, contact
// shadows, ambient occlusion, bloom, tonemap, FXAA, the sky LUTs) share: one copy each, so that two kernels which must agree on a pixel's clipmap, page or normal cannot drift apart.
// Every float operation keeps the order and rounding include/oxcull.h states; the including files are compiled without contraction.
#pragma once

#include "oxcull_device.hpp"

namespace oxc {

struct V3 {
  float x, y, z;
};

OXC_DEV V3 normalize3(const V3& v) {
  const float l = len3(v.x, v.y, v.z);
  return {v.x / l, v.y / l, v.z / l};
}

OXC_DEV int floor_mod_i(int x, int n) {
  const int r = x % n;
  return r < 0 ? r + n : r;
}
OXC_DEV float saturate_f(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }  // a NaN becomes 0 (max(NaN, 0) = 0)
OXC_DEV float sign_f(float a) { return a > 0.0f ? 1.0f : a < 0.0f ? -1.0f : 0.0f; }
OXC_DEV int clamp_i(int v, int lo, int hi) { return min(max(v, lo), hi); }

// mul(M, (x, y, z, 1)).r
OXC_DEV float row1(const float* m, int r, float x, float y, float z) { return ((OXC_M(m, r, 0) * x + OXC_M(m, r, 1) * y) + OXC_M(m, r, 2) * z) + OXC_M(m, r, 3); }

// binary32 -> binary16 bits, round to nearest even; the wave's FP16 denormal mode is at its default, so denormal halves are kept
OXC_DEV unsigned short f_to_half(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }
// binary16 bits of a colour channel: the same, every NaN the one pattern 0x7E00 (oxc_apply_pbr step 12; oxc_apply_bloom stores its RGBA16F
// levels by it)
OXC_DEV uint32_t channel_half(float x) { return x == x ? (uint32_t)f_to_half(x) : 0x7E00u; }

// ---- what the two G-buffer producers (oxcull_visbuffer_decode.hip, oxcull_terrain_decode.hip) share ----------------------------------------
constexpr uint32_t kTerrainInstanceId = 0xFFFFFEu;  // visbuffer.slang:16
constexpr uint32_t kHalfNaN = 0x7E00u;

// com::dequantize_half with the flush spelled out: an exponent field of 0 gives the sign alone (h in the low 16 bits)
OXC_DEV float dequantize_half_flush(uint32_t h) { return (h & 0x7C00u) ? dequantize_half(h) : asf((h & 0x8000u) << 16); }

// binary16 bits of a normal component: round to nearest even, denormals kept, every NaN the one pattern 0x7E00
OXC_DEV uint32_t normal_half(float x) { return x == x ? (uint32_t)f_to_half(x) : kHalfNaN; }

// com::vec3_to_oct (common/encoding.slang:17-21) as two normal halves, x in the low half (oxc_decode_visbuffer step 5)
OXC_DEV uint32_t oct_halves(const V3& n) {
  const float s = 1.0f / ((__builtin_fabsf(n.x) + __builtin_fabsf(n.y)) + __builtin_fabsf(n.z));
  const float ox = n.x * s, oy = n.y * s;
  const float sx = ox >= 0.0f ? 1.0f : -1.0f, sy = oy >= 0.0f ? 1.0f : -1.0f;
  const bool fold = n.z <= 0.0f;
  const float ex = fold ? (1.0f - __builtin_fabsf(oy)) * sx : ox, ey = fold ? (1.0f - __builtin_fabsf(ox)) * sy : oy;
  return normal_half(ex) | (normal_half(ey) << 16);
}

// the log2 rule before its rounding: binary64, no contraction
OXC_DEV double log2_f64(float x) {
  const uint32_t bits = asu(x);
  int e = (int)((bits >> 23) & 0xFFu) - 127;
  float m = asf((bits & 0x7FFFFFu) | 0x3F800000u);  // in [1, 2)
  const bool big = m > 1.41421356f;
  m = big ? m * 0.5f : m;  // exact
  e += big ? 1 : 0;
  const double f = (double)m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double p = 1.0 / 17.0;
  p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z + 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  p = p * z + 1.0;
  double r = (double)e + ((2.0 * s) * p) * 0x1.71547652b82fep+0;
  r = x >= 0x1p-126f ? r : -__builtin_inf();  // zero, denormal, negative, NaN
  return x == __builtin_inff() ? __builtin_inf() : r;
}

// exp2(y) of a binary64 y, rounded to binary32 once: the second half of the pow rule.  Host code runs the same expressions where a pass
// evaluates its pixel-independent constants (oxc_generate_sky_luts).
__host__ OXC_DEV float exp2_f64_round(double y) {
  const double k = __builtin_floor(y + 0.5);
  const double r = y - k;  // exact, in [-0.5, 0.5]
  const double t = r * 0x1.62e42fefa39efp-1;
  double q = 1.0 / 6227020800.0;
  q = q * t + 1.0 / 479001600.0;
  q = q * t + 1.0 / 39916800.0;
  q = q * t + 1.0 / 3628800.0;
  q = q * t + 1.0 / 362880.0;
  q = q * t + 1.0 / 40320.0;
  q = q * t + 1.0 / 5040.0;
  q = q * t + 1.0 / 720.0;
  q = q * t + 1.0 / 120.0;
  q = q * t + 1.0 / 24.0;
  q = q * t + 1.0 / 6.0;
  q = q * t + 1.0 / 2.0;
  q = q * t + 1.0;
  q = q * t + 1.0;
  if (y <= -160.0) return 0.0f;
  if (y >= 160.0) return __builtin_inff();
  if (!(y == y)) return __builtin_nanf("");
  const long long ki = (long long)k;  // in (-161, 161)
  const double scale = __builtin_bit_cast(double, (unsigned long long)(ki + 1023) << 52);
  return (float)(q * scale);
}

// pow(v, p), v >= 0 (or NaN-free by the caller's max), p > 0: exp2(p * log2(v)) in binary64, rounded to binary32 once
OXC_DEV float pow_rule(float v, float p) { return exp2_f64_round((double)p * log2_f64(v)); }

// exp2(t) of a binary32 t (the exp2 rule of oxc_apply_pbr)
OXC_DEV float exp2_rule(float t) { return exp2_f64_round((double)t); }

// exp(x) = exp2((double)x * log2(e)) (oxc_apply_tonemap step 6; the sky LUTs take every exp by it)
__host__ OXC_DEV float exp_rule(float x) { return exp2_f64_round((double)x * 0x1.71547652b82fep+0); }

// one component of packUnorm4x8: u32(floor(saturate(e) * 255.0 + 0.5)); a NaN gives 0
OXC_DEV uint32_t pack_unorm(float e) { return cvt_u32_sat(floorf(saturate_f(e) * 255.0f + 0.5f)); }

// the sRGB encoding of one linear channel, then unorm8 (oxc_decode_visbuffer step 6)
OXC_DEV uint32_t srgb_unorm(float x) {
  const float e = x <= 0.0031308f ? 12.92f * x : 1.055f * pow_rule(x, 1.0f / 2.4f) - 0.055f;
  return pack_unorm(e);
}

// the sRGB encoding of one colour channel before its unorm8 store (oxc_apply_tonemap step 11; the highlight composite stores by it too)
OXC_DEV float srgb_encode(float c) {
  c = saturate_f(c);
  return c <= 0.0031308f ? c * 12.92f : 1.055f * pow_rule(c, 0.4166666666666667f) - 0.055f;
}

// one channel of the sRGB decode (oxc_apply_pbr step 2; the Albedo debug view reads by it too)
OXC_DEV float srgb_decode(uint32_t byte) {
  const float c = (float)byte / 255.0f;
  return c <= 0.04045f ? c / 12.92f : pow_rule((c + 0.055f) / 1.055f, 2.4f);
}

// binary32 -> unsigned small float with a 5-bit exponent and MBITS of mantissa (UF11: 6, UF10: 5), truncating (oxc_decode_visbuffer
// step 8; oxc_apply_pbr packs its B10G11R11 output by it)
template <int MBITS>
OXC_DEV uint32_t pack_ufloat(float v) {
  constexpr uint32_t kMantissa = (1u << MBITS) - 1u;
  const uint32_t bits = asu(v);
  if (!(v == v)) return (31u << MBITS) | kMantissa;
  if (bits >> 31) return 0u;  // negative values, -0, -Inf
  if (bits == 0x7F800000u) return 31u << MBITS;
  const int e = (int)(bits >> 23) - 127 + 15;
  const uint32_t m = bits & 0x7FFFFFu;
  if (e >= 31) return (30u << MBITS) | kMantissa;
  if (e >= 1) return ((uint32_t)e << MBITS) | (m >> (23 - MBITS));
  const int sh = (23 - MBITS) + (1 - e);  // a denormal of the small format
  return sh > 24 ? 0u : (0x800000u | m) >> sh;
}

// unsigned small float with a 5-bit exponent and MBITS of mantissa -> binary32, exact (oxc_apply_pbr step 2; oxc_apply_eye_adaptation
// reads its B10G11R11 source by it)
template <int MBITS>
OXC_DEV float unpack_ufloat(uint32_t v) {
  const uint32_t e = v >> MBITS, m = v & ((1u << MBITS) - 1u);
  if (e == 0u) return (float)m * (MBITS == 6 ? 0x1p-20f : 0x1p-19f);
  if (e == 31u) return m ? __builtin_nanf("") : __builtin_inff();
  return asf(((e + 112u) << 23) | (m << (23 - MBITS)));
}

OXC_DEV float lerp_f(float a, float b, float t) { return a + (b - a) * t; }
OXC_DEV V3 lerp3(const V3& a, const V3& b, float t) { return {lerp_f(a.x, b.x, t), lerp_f(a.y, b.y, t), lerp_f(a.z, b.z, t)}; }

// A texel of the lit HDR image: B10G11R11 UfloatPack32 (FORMAT 0: the exact UF11 / UF11 / UF10 decode, alpha 1.0) or R16G16B16A16 Sfloat
// (FORMAT 1: four halves, exact, denormals kept)
struct Texel {
  V3 c;
  float a;
};
template <int FORMAT>
OXC_DEV Texel load_rgba(const void* base, size_t i) {
  if (FORMAT == 0) {
    const uint32_t w = static_cast<const uint32_t*>(base)[i];
    return {{unpack_ufloat<6>(w & 0x7FFu), unpack_ufloat<6>((w >> 11) & 0x7FFu), unpack_ufloat<5>(w >> 22)}, 1.0f};
  }
  const uint2 v = static_cast<const uint2*>(base)[i];
  return {{dequantize_half(v.x & 0xFFFFu), dequantize_half(v.x >> 16), dequantize_half(v.y & 0xFFFFu)}, dequantize_half(v.y >> 16)};
}

// One axis of a manual bilinear tap (the oxc_apply_bloom block): the two texel coordinates, whether each lies inside the level (border
// mode; a coordinate outside is stored as 0 and not loaded) and the weight of the second.
struct Axis {
  int i0, i1;
  bool in0, in1;
  float f;
};
// p the normalised coordinate of the tap, fsize / last the source level's side.  Clamp mode (BORDER false): both coordinates lie in
// [0, last] for every bit pattern of p (a NaN converts to 0, +-Inf saturates).
template <bool BORDER>
OXC_DEV Axis axis_at(float p, float fsize, int last) {
  const float g = p * fsize - 0.5f;
  const float fl = floorf(g);
  const int i = clamp_i(cvt_i32_sat(fl), -2, last + 1);  // i + 1 cannot wrap after this, and what lay outside [-1, last] still does
  Axis a;
  a.f = g - fl;
  if (BORDER) {
    a.in0 = i >= 0 && i <= last;
    a.in1 = i + 1 >= 0 && i + 1 <= last;
    a.i0 = a.in0 ? i : 0;
    a.i1 = a.in1 ? i + 1 : 0;
  } else {
    a.in0 = a.in1 = true;
    a.i0 = clamp_i(i, 0, last);
    a.i1 = clamp_i(i + 1, 0, last);
  }
  return a;
}

// One axis of a repeat-mode bilinear tap at the normalised coordinate `coord` of a level `size` texels wide: both texel coordinates lie in
// [0, size - 1] for every bit pattern of `coord` (a NaN converts to 0, +-Inf saturates).  oxc_apply_tonemap's bloom and lens taps and the
// repeat address mode of oxc_decode_visbuffer_textured.
struct WrapAxis {
  int i0, i1;
  float f;
};
OXC_DEV WrapAxis wrap_axis(float coord, int size) {
  const float g = coord * (float)size - 0.5f;
  const float fl = floorf(g);
  WrapAxis a;
  a.i0 = floor_mod_i(cvt_i32_sat(fl), size);
  a.i1 = a.i0 + 1 == size ? 0 : a.i0 + 1;
  a.f = g - fl;
  return a;
}

// The pixel of this thread: an 8 x 8 pixel tile per wave, a 16 x 16 tile per block of 256 threads.
OXC_DEV uint2 tile_pixel() {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  return make_uint2(blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u), blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3));
}

// mul(m, (u * 2 - 1, v * 2 - 1, d, 1)).xyz / .w
OXC_DEV void unproject(const float* m, float u, float v, float d, float& x, float& y, float& z) {
  const float nx = u * 2.0f - 1.0f, ny = v * 2.0f - 1.0f;
  const float hx = ((OXC_M(m, 0, 0) * nx + OXC_M(m, 0, 1) * ny) + OXC_M(m, 0, 2) * d) + OXC_M(m, 0, 3);
  const float hy = ((OXC_M(m, 1, 0) * nx + OXC_M(m, 1, 1) * ny) + OXC_M(m, 1, 2) * d) + OXC_M(m, 1, 3);
  const float hz = ((OXC_M(m, 2, 0) * nx + OXC_M(m, 2, 1) * ny) + OXC_M(m, 2, 2) * d) + OXC_M(m, 2, 3);
  const float hw = ((OXC_M(m, 3, 0) * nx + OXC_M(m, 3, 1) * ny) + OXC_M(m, 3, 2) * d) + OXC_M(m, 3, 3);
  x = hx / hw;
  y = hy / hw;
  z = hz / hw;
}

// The wrapped page coordinate of clipmap uv (su, sv) in [0, 1]^2, `c` the clipmap's record (its page offsets in c[16], c[17]), fn = (float)n;
// false for uv == 1.0, which lands on virt == n.
OXC_DEV bool wrapped_page(const float* c, float su, float sv, float fn, int n, uint32_t& wx, uint32_t& wy) {
  const int vx = (int)floorf(su * fn), vy = (int)floorf(sv * fn);
  if (vx > n - 1 || vy > n - 1) return false;
  const int ox = __builtin_bit_cast(int, c[16]), oy = __builtin_bit_cast(int, c[17]);
  wx = (uint32_t)floor_mod_i(vx + floor_mod_i(ox, n), n);
  wy = (uint32_t)floor_mod_i(vy + floor_mod_i(oy, n), n);
  return true;
}

// oct_to_vec3(normal.ba) before any normalisation; `nba` = the texel's second word, .b in the low half, .a in the high half
OXC_DEV V3 oct_normal_ba(uint32_t nba) {
  const float ex = dequantize_half(nba & 0xFFFFu), ey = dequantize_half(nba >> 16);
  V3 o;
  o.z = (1.0f - __builtin_fabsf(ex)) - __builtin_fabsf(ey);
  const float sx = ex >= 0.0f ? 1.0f : -1.0f, sy = ey >= 0.0f ? 1.0f : -1.0f;
  const bool fold = o.z < 0.0f;
  o.x = fold ? (1.0f - __builtin_fabsf(ey)) * sx : ex;
  o.y = fold ? (1.0f - __builtin_fabsf(ex)) * sy : ey;
  return o;
}

// com::oct_to_vec3 of the two halves of `word` (the first in the low half): one normalisation
OXC_DEV V3 oct_to_vec3(uint32_t word) { return normalize3(oct_normal_ba(word)); }

// The world position and the clipmap index of pixel (u, v) at depth d (oxc_resolve_shadowmap step 2): `a` carries inv_pv, the footprint
// offsets, texel_len and the level thresholds of clipmap_selection_constants.  One copy for the resolve and the RMVSM debug view, which
// must agree with the page update's pixel_page (oxcull_vsm.hip) on every pixel's clipmap.
template <class Args>
OXC_DEV int pixel_world_and_clipmap(const Args& a, float u, float v, float d, V3& world) {
  V3 lf, rt;
  unproject(a.inv_pv, u, v, d, world.x, world.y, world.z);
  unproject(a.inv_pv, u + -a.off_x, v + a.off_y, d, lf.x, lf.y, lf.z);
  unproject(a.inv_pv, u + a.off_x, v + a.off_y, d, rt.x, rt.y, rt.z);
  const float r = len3(lf.x - rt.x, lf.y - rt.y, lf.z - rt.z) / a.texel_len;
  uint32_t idx = a.lvl_always;
  for (uint32_t k = a.lvl_always; k + 1 < a.layers; k++) idx += (r > a.lvl_thr[k]) ? 1u : 0u;  // NaN: never
  return (int)idx;
}

// (cos, sin) of 2 pi t, t a binary32 in [0, 1): exact reduction to an octant, two binary64 polynomials by Horner, one rounding each
// (the rotation rule of oxc_resolve_shadowmap, step 6 of its header block; oxc_generate_ambient_occlusion turns its slices by it too).
OXC_DEV void cos_sin_turn(float t, float& cs, float& sn) {
  const float q4 = t * 4.0f;  // exact
  const float kf = floorf(q4);
  const float f = q4 - kf;  // exact, in [0, 1)
  const bool swap = f > 0.5f;
  const float g = swap ? 1.0f - f : f;  // exact, in [0, 0.5]
  const double a = (double)g * 0x1.921fb54442d18p+0;
  const double z = a * a;
  const double ps = ((0x1.71de3a556c734p-19 * z + -0x1.a01a01a01a01ap-13) * z + 0x1.1111111111111p-7) * z + -0x1.5555555555555p-3;
  const double s = a + (a * z) * ps;
  const double pc = (((-0x1.27e4fb7789f5cp-22 * z + 0x1.a01a01a01a01ap-16) * z + -0x1.6c16c16c16c17p-10) * z + 0x1.5555555555555p-5) * z + -0x1.0000000000000p-1;
  const double c = 1.0 + z * pc;
  const float sf = (float)s, cf = (float)c;
  const float sq = swap ? cf : sf, cq = swap ? sf : cf;
  const int k = (int)kf;
  cs = k == 0 ? cq : k == 1 ? -sq : k == 2 ? -cq : sq;
  sn = k == 0 ? sq : k == 1 ? cq : k == 2 ? -sq : -cq;
}

// cos(a) of a binary32 angle in radians (oxc_apply_tonemap step 6; oxc_draw_atmosphere turns its view directions by it): NaN for a
// non-finite a; else u = (double)|a| / (2 pi), t = (float)(u - floor(u)), t == 1 becomes 0, the cosine of the turn t
OXC_DEV float cos_turn_rule(float a) {
  const float aa = __builtin_fabsf(a);
  const double u = (double)aa * 0x1.45f306dc9c883p-3;
  float t = (float)(u - __builtin_floor(u));
  t = t == 1.0f ? 0.0f : t;
  t = aa < __builtin_inff() ? t : 0.0f;  // a non-finite argument: any turn, the result is replaced below
  float cs, sn;
  cos_sin_turn(t, cs, sn);
  return aa < __builtin_inff() ? cs : __builtin_nanf("");
}

// (cos(a), sin(a)) of a binary32 angle in radians (oxc_generate_sky_ibl step 11): the turn of the cos rule above, so cs is cos_turn_rule(a)
// bit for bit; the sine of that turn, negated for a < 0.  Both NaN for a non-finite a.
OXC_DEV void cos_sin_angle_rule(float a, float& cs, float& sn) {
  const float aa = __builtin_fabsf(a);
  const double u = (double)aa * 0x1.45f306dc9c883p-3;
  float t = (float)(u - __builtin_floor(u));
  t = t == 1.0f ? 0.0f : t;
  t = aa < __builtin_inff() ? t : 0.0f;
  cos_sin_turn(t, cs, sn);
  sn = a < 0.0f ? -sn : sn;
  cs = aa < __builtin_inff() ? cs : __builtin_nanf("");
  sn = aa < __builtin_inff() ? sn : __builtin_nanf("");
}

// atan2(y, x) before its rounding (oxc_generate_sky_ibl step 11), binary64 throughout, no contraction: a = min(|x|, |y|) / max(|x|, |y|);
// a > sqrt(2) - 1 is reduced by atan(a) = pi / 4 + atan((a - 1) / (a + 1)); 20 terms of the odd series by Horner; the octant, then the
// quadrant by `x < 0` and `y < 0` (a negative zero counts as positive).  (0, 0) gives 0; a NaN argument, or two infinite ones, NaN.
OXC_DEV double atan2_f64(double y, double x) {
  const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
  const double mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
  const double a = mn / mx;
  const bool fold = a > 0x1.a827999fcef32p-2;
  const double t = fold ? (a - 1.0) / (a + 1.0) : a;
  const double z = t * t;
  double p = 1.0 / 39.0;
  p = 1.0 / 37.0 - p * z;
  p = 1.0 / 35.0 - p * z;
  p = 1.0 / 33.0 - p * z;
  p = 1.0 / 31.0 - p * z;
  p = 1.0 / 29.0 - p * z;
  p = 1.0 / 27.0 - p * z;
  p = 1.0 / 25.0 - p * z;
  p = 1.0 / 23.0 - p * z;
  p = 1.0 / 21.0 - p * z;
  p = 1.0 / 19.0 - p * z;
  p = 1.0 / 17.0 - p * z;
  p = 1.0 / 15.0 - p * z;
  p = 1.0 / 13.0 - p * z;
  p = 1.0 / 11.0 - p * z;
  p = 1.0 / 9.0 - p * z;
  p = 1.0 / 7.0 - p * z;
  p = 1.0 / 5.0 - p * z;
  p = 1.0 / 3.0 - p * z;
  p = 1.0 - p * z;
  double r = t * p;
  r = fold ? 0x1.921fb54442d18p-1 + r : r;
  r = ay > ax ? 0x1.921fb54442d18p+0 - r : r;
  r = x < 0.0 ? 0x1.921fb54442d18p+1 - r : r;
  r = y < 0.0 ? -r : r;
  r = mx == 0.0 ? 0.0 : r;
  return (x == x && y == y) ? r : __builtin_nan("");
}

// atan2(y, x) of two binary32, rounded to binary32 once
OXC_DEV float atan2_rule(float y, float x) { return (float)atan2_f64((double)y, (double)x); }

// acos(x) of a binary32 x: atan2(sqrt(1 - x * x), x) in binary64 (x * x is exact there), rounded to binary32 once; NaN for a NaN and for
// |x| > 1.  acos(1) = 0, acos(-1) = (float)pi, acos(0) = (float)(pi / 2).
OXC_DEV float acos_rule(float x) {
  const double xd = (double)x;
  const float r = (float)atan2_f64(__builtin_sqrt(1.0 - xd * xd), xd);
  return __builtin_fabsf(x) <= 1.0f ? r : __builtin_nanf("");
}

// ---- what the sky passes (oxcull_atmosphere.hip) and the atmosphere branch of apply_pbr (oxcull_pbr_apply.hip) share ------------------------------
OXC_DEV float dot3v(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
OXC_DEV V3 crossv(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
OXC_DEV float safe_sqrt(float x) { return __builtin_sqrtf(fmaxf(0.0f, x)); }

// com::ray_sphere_intersect_nearest (common/math.slang:104-138); `value` is 0.0 where the Slang's Optional is none
struct Hit {
  bool has;
  float value;
};
OXC_DEV Hit intersect_nearest(const V3& o, const V3& d, float radius) {
  const float a = dot3v(d, d), b = 2.0f * dot3v(d, o), c = dot3v(o, o) - radius * radius;
  const float delta = b * b - (4.0f * a) * c;
  if (delta < 0.0f) return {false, 0.0f};
  const float sq = __builtin_sqrtf(delta), den = 2.0f * a;
  const float s0 = (-b + -1.0f * sq) / den, s1 = (-b + sq) / den;
  if (s0 < 0.0f && s1 < 0.0f) return {false, 0.0f};
  if (s0 < 0.0f) return {true, fmaxf(0.0f, s1)};
  if (s1 < 0.0f) return {true, fmaxf(0.0f, s0)};
  return {true, fmaxf(0.0f, fminf(s0, s1))};
}

// SampleLevel(LinearSamplerClamped, uv, 0).rgb of a w x h RGBA16F LUT: the manual bilinear of the oxc_apply_bloom block, clamp mode
OXC_DEV V3 sample_rgb(const uint2* lut, uint32_t w, uint32_t h, float u, float v) {
  const Axis ax = axis_at<false>(u, (float)w, (int)w - 1), ay = axis_at<false>(v, (float)h, (int)h - 1);
  const size_t r0 = (size_t)ay.i0 * w, r1 = (size_t)ay.i1 * w;
  const V3 t00 = load_rgba<1>(lut, r0 + ax.i0).c, t10 = load_rgba<1>(lut, r0 + ax.i1).c;
  const V3 t01 = load_rgba<1>(lut, r1 + ax.i0).c, t11 = load_rgba<1>(lut, r1 + ax.i1).c;
  return lerp3(lerp3(t00, t10, ax.f), lerp3(t01, t11, ax.f), ay.f);
}

// ... with its alpha: the same bilinear on all four channels
OXC_DEV Texel sample_rgba(const uint2* lut, uint32_t w, uint32_t h, float u, float v) {
  const Axis ax = axis_at<false>(u, (float)w, (int)w - 1), ay = axis_at<false>(v, (float)h, (int)h - 1);
  const size_t r0 = (size_t)ay.i0 * w, r1 = (size_t)ay.i1 * w;
  const Texel t00 = load_rgba<1>(lut, r0 + ax.i0), t10 = load_rgba<1>(lut, r0 + ax.i1);
  const Texel t01 = load_rgba<1>(lut, r1 + ax.i0), t11 = load_rgba<1>(lut, r1 + ax.i1);
  return {lerp3(lerp3(t00.c, t10.c, ax.f), lerp3(t01.c, t11.c, ax.f), ay.f), lerp_f(lerp_f(t00.a, t10.a, ax.f), lerp_f(t01.a, t11.a, ax.f), ay.f)};
}

// transmittance_params_to_lut_uv (sky.slang:15-29) at (h, mu) and the sample there: step 3 of the sky LUT block; h_atmos the host constant H
OXC_DEV V3 transmittance_sample(const uint2* lut, uint32_t w, uint32_t hgt, float planet_radius, float atmos_radius, float h_atmos, float h, float mu) {
  const float rho = safe_sqrt(h * h - planet_radius * planet_radius);
  const float discriminant = (h * h) * (mu * mu - 1.0f) + atmos_radius * atmos_radius;
  const float d = fmaxf(0.0f, -h * mu + safe_sqrt(discriminant));
  const float d_min = atmos_radius - h, d_max = rho + h_atmos;
  return sample_rgb(lut, w, hgt, (d - d_min) / (d_max - d_min), rho / h_atmos);
}

// sky_view_params_to_lut_uv (sky.slang:39-67) with the host constants zenith_horizon_angle and beta: step 14 of oxc_generate_sky_ibl
OXC_DEV void sky_view_lut_uv(float zha, float beta, uint32_t w, uint32_t hgt, bool intersect_planet, float view_zenith_cos_angle, float lx, float ly, float& u, float& v) {
  const float view_zenith_angle = acos_rule(view_zenith_cos_angle);
  float uy;
  if (!intersect_planet) {
    float coord = view_zenith_angle / zha;
    coord = 1.0f - coord;
    coord = safe_sqrt(coord);
    coord = 1.0f - coord;
    uy = coord * 0.5f;
  } else {
    float coord = (view_zenith_angle - zha) / beta;
    coord = safe_sqrt(coord);
    uy = coord * 0.5f + 0.5f;
  }
  const float pi = 3.1415926535897932384626433832795f;
  const float theta = atan2_rule(-ly, -lx);
  const float ux = (theta + pi) / (2.0f * pi);
  const float fw = (float)w, fh = (float)hgt;
  u = (ux + 0.5f / fw) * (fw / (fw + 1.0f));
  v = (uy + 0.5f / fh) * (fh / (fh + 1.0f));
}

}  // namespace oxc
