// oxcull_tonemap.hip -- exposure, bloom composite, tone curve, lens effects and the 8-bit store (gfx950): RendererInstance::apply_tonemap
// (Oxylus/src/Render/Passes/PostProcess.cpp:205-247, passes/tonemap.slang, passes/lens.slang, common/color.slang:4-55).  Rules:
// include/oxcull.h, oxc_apply_tonemap; design and measurements: DESIGN.md section 19.
//
//   k_tonemap<TONEMAP, FORMAT>  one thread per pixel, 16 x 16 pixels per block from tile_pixel().  The tone curve and the source format are
//                 template parameters (the reference specialises its pipeline on the curve too); the scene flags and the output format are
//                 wave-uniform branches on kernel arguments.  One launch, no LDS, no scratch.
//
// Step 5 of the header: whatever of the curves and of FfxLensGetRGMag does not depend on the pixel is evaluated once per call on the
// host by tonemap_constants() below -- binary32 in the Slang's order, this file being compiled without contraction for the host as for the
// device -- and reaches the kernel in TonemapArgs::k.  The host needs log2 / exp2 / pow of oxcull_pixel_device.hpp for three of them (kB_,
// framebufferLuminanceTargetUcs_): exp2 and exp are the header's own functions, compiled for the host too; host_rules holds log2 as plain
// C++, and tests/test_gpu_tonemap.py pins the two against the checker's constants through every GT7 pixel.  The exp and cos rules are those of oxcull_pixel_device.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr double kLog2E = 0x1.71547652b82fep+0;
// eotfSt2084 / inverseEotfSt2084 (tonemap.slang:403-408): every one exact in binary32 but m1 and its kin, which are literals
constexpr float kPqM1 = 0.1593017578125f, kPqC1 = 0.8359375f, kPqC2 = 18.8515625f, kPqC3 = 18.6875f, kPqC = 10000.0f;
constexpr float kReferenceLuminance = 100.0f, kSdrPaperWhite = 250.0f;

// ---- the host's side of the log2 / exp2 rules, for tonemap_constants: exp2_f64_round and exp_rule are the shared host-and-device functions of
// oxcull_pixel_device.hpp; log2_f64 there takes its bits through device-only casts, so the host keeps this one copy of it ---------------------------
namespace host_rules {
double log2_f64(float x) {
  uint32_t bits;
  std::memcpy(&bits, &x, 4);
  int e = (int)((bits >> 23) & 0xFFu) - 127;
  const uint32_t mb = (bits & 0x7FFFFFu) | 0x3F800000u;
  float m;
  std::memcpy(&m, &mb, 4);
  const bool big = m > 1.41421356f;
  m = big ? m * 0.5f : m;
  e += big ? 1 : 0;
  const double f = (double)m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double p = 1.0 / 17.0;
  for (double c : {1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0, 1.0}) p = p * z + c;
  double r = (double)e + ((2.0 * s) * p) * kLog2E;
  r = x >= 0x1p-126f ? r : -HUGE_VAL;
  return x == HUGE_VALF ? HUGE_VAL : r;
}
float pow_rule(float v, float p) { return exp2_f64_round((double)p * log2_f64(v)); }
float log2_rule(float x) { return (float)log2_f64(x); }
float exp2_rule(float t) { return exp2_f64_round((double)t); }
float inverse_eotf(float v, float m2) {
  const float y = (v * kReferenceLuminance) / kPqC;
  const float ym = pow_rule(y, kPqM1);
  return exp2_rule(m2 * (log2_rule(kPqC1 + kPqC2 * ym) - log2_rule(1.0f + kPqC3 * ym)));
}

struct M3 {
  float m[3][3];
};
// inverse() of tonemap.slang:131-155
M3 inverse(const M3& in) {
  const float a = in.m[0][0], b = in.m[0][1], c = in.m[0][2], d = in.m[1][0], e = in.m[1][1], f = in.m[1][2], g = in.m[2][0], h = in.m[2][1], i = in.m[2][2];
  const float A = (e * i - f * h), B = -(d * i - f * g), C = (d * h - e * g), D = -(b * i - c * h), E = (a * i - c * g), F = -(a * h - b * g);
  const float G = (b * f - c * e), H = -(a * f - c * d), I = (a * e - b * d);
  const float det = (a * A + b * B) + c * C;
  const float inv = 1.0f / det;
  return {{{A * inv, D * inv, G * inv}, {B * inv, E * inv, H * inv}, {C * inv, F * inv, I * inv}}};
}
struct XY {
  float x, y;
};
struct XYZ {
  float x, y, z;
};
// color_Unproject: color_XyYToXYZ((x, y, 1.0))
XYZ unproject(XY p) {
  const float Y = 1.0f;
  return {(p.x * Y) / p.y, Y, (((1.0f - p.x) - p.y) * Y) / p.y};
}
M3 primaries_to_matrix(XY r, XY g, XY b, XY w) {
  const XYZ R = unproject(r), G = unproject(g), B = unproject(b), W = unproject(w);
  const M3 temp = {{{R.x, G.x, B.x}, {1.0f, 1.0f, 1.0f}, {R.z, G.z, B.z}}};
  const M3 inv = inverse(temp);
  float scale[3];
  for (int k = 0; k < 3; k++) scale[k] = (inv.m[k][0] * W.x + inv.m[k][1] * W.y) + inv.m[k][2] * W.z;
  return {{{R.x * scale[0], G.x * scale[1], B.x * scale[2]}, {R.y * scale[0], G.y * scale[1], B.y * scale[2]}, {R.z * scale[0], G.z * scale[1], B.z * scale[2]}}};
}
XY lerp_xy(XY a, XY b, float t) { return {a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t}; }
}  // namespace host_rules
}  // namespace

float pow_rule_host(float v, float p) { return host_rules::pow_rule(v, p); }

void tonemap_constants(float chromatic_aberration_amount, TonemapConstants& k) {
  using host_rules::M3;
  using host_rules::XY;
  using host_rules::inverse;
  using host_rules::lerp_xy;
  using host_rules::primaries_to_matrix;
  // AgX_DS (tonemap.slang:227-262)
  const XY xr = {0.64f, 0.33f}, xg = {0.3f, 0.6f}, xb = {0.15f, 0.06f}, xw = {0.3127f, 0.3290f};
  const M3 srgb_to_xyz = primaries_to_matrix(xr, xg, xb, xw);
  const float scale_factor = 1.0f / (1.0f - 0.15f);
  const M3 adjusted_to_xyz = primaries_to_matrix(lerp_xy(xw, xr, scale_factor), lerp_xy(xw, xg, scale_factor), lerp_xy(xw, xb, scale_factor), xw);
  const M3 xyz_to_adjusted = inverse(adjusted_to_xyz);
  M3 srgb_to_adjusted;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      srgb_to_adjusted.m[r][c] = (srgb_to_xyz.m[r][0] * xyz_to_adjusted.m[0][c] + srgb_to_xyz.m[r][1] * xyz_to_adjusted.m[1][c]) + srgb_to_xyz.m[r][2] * xyz_to_adjusted.m[2][c];
  const M3 back = inverse(srgb_to_adjusted);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) k.agx_in[r * 3 + c] = srgb_to_adjusted.m[r][c], k.agx_out[r * 3 + c] = back.m[r][c];
  const float agx_peak = 1.0f, agx_linear = 0.10f;
  k.agx_peak = agx_peak;
  k.agx_s = agx_peak * agx_linear;
  k.agx_span = agx_peak - k.agx_s;
  k.agx_neg_c = -(agx_peak / k.agx_span);
  // GT7ToneMapping::initializeAsSDR (tonemap.slang:576-624), GTToneMappingCurveV2::initializeCurve (:339-356)
  k.gt_sdr = 1.0f / (kSdrPaperWhite / kReferenceLuminance);
  k.gt_target = kSdrPaperWhite / kReferenceLuminance;
  const float alpha = 0.25f, mid = 0.538f, lin = 0.444f, toe = 1.280f;
  const float kk = (lin - 1.0f) / (alpha - 1.0f);
  k.gt_mid = mid;
  k.gt_toe = toe;
  k.gt_ka = k.gt_target * lin + k.gt_target * kk;
  k.gt_kb = (-k.gt_target * kk) * exp_rule(lin / kk);
  k.gt_kc = -1.0f / (kk * k.gt_target);
  k.gt_lin_peak = lin * k.gt_target;
  k.gt_mid_span = mid - 0.0f;
  k.gt_blend = 0.6f;
  k.gt_one_minus_blend = 1.0f - 0.6f;
  k.gt_fade_start = 0.98f;
  k.gt_fade_end = 1.16f;
  k.gt_fade_span = 1.16f - 0.98f;
  k.pq_m2 = 78.84375f * 1.0f;
  k.pq_inv_m2 = 1.0f / k.pq_m2;
  k.pq_inv_m1 = 1.0f / kPqM1;
  {  // rgbToICtCp((target, target, target))[0]
    const float t = k.gt_target;
    const float l = ((t * 1688.0f + t * 2146.0f) + t * 262.0f) / 4096.0f, m = ((t * 683.0f + t * 2951.0f) + t * 462.0f) / 4096.0f;
    k.gt_target_ucs = (2048.0f * host_rules::inverse_eotf(l, k.pq_m2) + 2048.0f * host_rules::inverse_eotf(m, k.pq_m2)) / 4096.0f;
  }
  // FfxLensGetRGMag (lens.slang:51-67)
  const float A = 1.5220f, B = 0.00459f * chromatic_aberration_amount;
  const float red = A + B / (0.612f * 0.612f), green = A + B / (0.549f * 0.549f), blue = A + B / (0.464f * 0.464f);
  k.red_mag = (red - 1.0f) / (blue - 1.0f);
  k.green_mag = (green - 1.0f) / (blue - 1.0f);
}

namespace {
// ---- step 6: the log2 rule rounded to binary32 (exp and cos: oxcull_pixel_device.hpp) ---------------------------------------------------------
OXC_DEV float log2_rule(float x) { return (float)log2_f64(x); }

OXC_DEV V3 mul_mv(const float* m, const V3& v) {
  return {(m[0] * v.x + m[1] * v.y) + m[2] * v.z, (m[3] * v.x + m[4] * v.y) + m[5] * v.z, (m[6] * v.x + m[7] * v.y) + m[8] * v.z};
}
OXC_DEV float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// ---- step 4: ACES_Fitted (tonemap.slang:37-69) -----------------------------------------------------------------------------------------------
OXC_DEV float rrt_odt_fit(float v) {
  const float a = v * (v + 0.0245786f) - 0.000090537f;
  const float b = v * (0.983729f * v + 0.4329510f) + 0.238081f;
  return a / b;
}
OXC_DEV V3 aces_fitted(V3 c) {
  const float in[9] = {0.59719f, 0.35458f, 0.04823f, 0.07600f, 0.90834f, 0.01566f, 0.02840f, 0.13383f, 0.83777f};
  const float out[9] = {1.60475f, -0.53108f, -0.07367f, -0.10208f, 1.10813f, -0.00605f, -0.00327f, -0.07276f, 1.07602f};
  c = mul_mv(in, c);
  c = {rrt_odt_fit(c.x), rrt_odt_fit(c.y), rrt_odt_fit(c.z)};
  c = mul_mv(out, c);
  return {saturate_f(c.x), saturate_f(c.y), saturate_f(c.z)};
}

// ---- step 4: AgX_DS (tonemap.slang:204-262) --------------------------------------------------------------------------------------------------
OXC_DEV float dual_section(float x, const TonemapConstants& k) {
  if (x < k.agx_s) return x;
  return k.agx_peak - k.agx_span * exp_rule((k.agx_neg_c * (x - k.agx_s)) / k.agx_peak);
}
OXC_DEV V3 agx_ds(V3 c, const TonemapConstants& k) {
  V3 w = {fmaxf(c.x, 0.0f), fmaxf(c.y, 0.0f), fmaxf(c.z, 0.0f)};
  w = mul_mv(k.agx_in, w);
  w = {clamp01(dual_section(w.x, k)), clamp01(dual_section(w.y, k)), clamp01(dual_section(w.z, k))};
  const float d = (w.x * 0.2126729f + w.y * 0.7151522f) + w.z * 0.0721750f;
  w = {clamp01(d + (w.x - d) * 1.3f), clamp01(d + (w.y - d) * 1.3f), clamp01(d + (w.z - d) * 1.3f)};
  return mul_mv(k.agx_out, w);
}

// ---- step 4: GT7 (tonemap.slang:267-666) -----------------------------------------------------------------------------------------------------
OXC_DEV float smooth_step(float x, float edge0, float edge1, float span) {
  const float t = (x - edge0) / span;
  if (x < edge0) return 0.0f;
  if (x > edge1) return 1.0f;
  return (t * t) * (3.0f - 2.0f * t);
}
OXC_DEV float gt_curve(float x, const TonemapConstants& k) {
  if (x < 0.0f) return 0.0f;
  const float weight_linear = smooth_step(x, 0.0f, k.gt_mid, k.gt_mid_span);
  const float weight_toe = 1.0f - weight_linear;
  if (x < k.gt_lin_peak) {
    const float toe_mapped = k.gt_mid * pow_rule(x / k.gt_mid, k.gt_toe);
    return weight_toe * toe_mapped + weight_linear * x;
  }
  return k.gt_ka + k.gt_kb * exp_rule(x * k.gt_kc);
}
OXC_DEV float inverse_eotf(float v, const TonemapConstants& k) {
  const float y = (v * kReferenceLuminance) / kPqC;
  const float ym = pow_rule(y, kPqM1);  // a negative, zero, denormal or NaN y gives 0
  return exp2_rule(k.pq_m2 * (log2_rule(kPqC1 + kPqC2 * ym) - log2_rule(1.0f + kPqC3 * ym)));
}
OXC_DEV float eotf(float n, const TonemapConstants& k) {
  n = n < 0.0f ? 0.0f : n;
  n = n > 1.0f ? 1.0f : n;
  const float np = pow_rule(n, k.pq_inv_m2);
  float l = np - kPqC1;
  l = l < 0.0f ? 0.0f : l;
  l = l / (kPqC2 - kPqC3 * np);
  l = pow_rule(l, k.pq_inv_m1);
  return (l * kPqC) / kReferenceLuminance;
}
OXC_DEV void lms_pq(const V3& rgb, const TonemapConstants& k, float& lp, float& mp, float& sp, bool with_s) {
  const float l = ((rgb.x * 1688.0f + rgb.y * 2146.0f) + rgb.z * 262.0f) / 4096.0f;
  const float m = ((rgb.x * 683.0f + rgb.y * 2951.0f) + rgb.z * 462.0f) / 4096.0f;
  const float s = ((rgb.x * 99.0f + rgb.y * 309.0f) + rgb.z * 3688.0f) / 4096.0f;
  lp = inverse_eotf(l, k);
  mp = inverse_eotf(m, k);
  sp = with_s ? inverse_eotf(s, k) : 0.0f;
}
OXC_DEV V3 gt7_apply(const V3& rgb, const TonemapConstants& k) {
  float lp, mp, sp;
  lms_pq(rgb, k, lp, mp, sp, true);
  const float ucs0 = (2048.0f * lp + 2048.0f * mp) / 4096.0f;
  const float ucs1 = ((6610.0f * lp - 13613.0f * mp) + 7003.0f * sp) / 4096.0f;
  const float ucs2 = ((17933.0f * lp - 17390.0f * mp) - 543.0f * sp) / 4096.0f;
  const V3 skewed = {gt_curve(rgb.x, k), gt_curve(rgb.y, k), gt_curve(rgb.z, k)};
  lms_pq(skewed, k, lp, mp, sp, false);  // only I of the skewed colour is read
  const float skewed0 = (2048.0f * lp + 2048.0f * mp) / 4096.0f;
  const float chroma = 1.0f - smooth_step(ucs0 / k.gt_target_ucs, k.gt_fade_start, k.gt_fade_end, k.gt_fade_span);
  const float ct = ucs1 * chroma, cp = ucs2 * chroma;
  const float l = (skewed0 + 0.00860904f * ct) + 0.11103f * cp;
  const float m = (skewed0 - 0.00860904f * ct) - 0.11103f * cp;
  const float s = (skewed0 + 0.560031f * ct) - 0.320627f * cp;
  const float ll = eotf(l, k), ml = eotf(m, k), sl = eotf(s, k);
  const V3 scaled = {fmaxf((3.43661f * ll - 2.50645f * ml) + 0.0698454f * sl, 0.0f), fmaxf((-0.79133f * ll + 1.9836f * ml) - 0.192271f * sl, 0.0f),
                     fmaxf((-0.0259499f * ll - 0.0989137f * ml) + 1.12486f * sl, 0.0f)};
  return {k.gt_sdr * fminf(k.gt_one_minus_blend * skewed.x + k.gt_blend * scaled.x, k.gt_target),
          k.gt_sdr * fminf(k.gt_one_minus_blend * skewed.y + k.gt_blend * scaled.y, k.gt_target),
          k.gt_sdr * fminf(k.gt_one_minus_blend * skewed.z + k.gt_blend * scaled.z, k.gt_target)};
}
OXC_DEV V3 gt7(const V3& c, const TonemapConstants& k) {
  const float rec709_to_xyz[9] = {0.4124564f, 0.3575761f, 0.1804375f, 0.2126729f, 0.7151522f, 0.0721750f, 0.0193339f, 0.1191920f, 0.9503041f};
  const float xyz_to_rec709[9] = {3.2404542f, -1.5371385f, -0.4985314f, -0.9692660f, 1.8760108f, 0.0415560f, 0.0556434f, -0.2040259f, 1.0572252f};
  const float rec2020_to_xyz[9] = {0.636958f, 0.1446169f, 0.168881f, 0.2627002f, 0.6779981f, 0.0593017f, 0.0f, 0.0280727f, 1.0609851f};
  const float xyz_to_rec2020[9] = {1.7166512f, -0.3556708f, -0.2533663f, -0.6666844f, 1.6164812f, 0.0157685f, 0.0176399f, -0.0427706f, 0.9421031f};
  return mul_mv(xyz_to_rec709, mul_mv(rec2020_to_xyz, gt7_apply(mul_mv(xyz_to_rec2020, mul_mv(rec709_to_xyz, c)), k)));
}

// ---- sampling --------------------------------------------------------------------------------------------------------------------------------
// channel CH of texel i
template <int FORMAT, int CH>
OXC_DEV float load_channel(const void* base, size_t i) {
  if (FORMAT == 0) {
    const uint32_t w = static_cast<const uint32_t*>(base)[i];
    return CH == 0 ? unpack_ufloat<6>(w & 0x7FFu) : CH == 1 ? unpack_ufloat<6>((w >> 11) & 0x7FFu) : unpack_ufloat<5>(w >> 22);
  }
  return dequantize_half(static_cast<const unsigned short*>(base)[i * 4u + CH]);
}

template <int FORMAT, int CH>
OXC_DEV float tap_channel(const void* src, int sw, int sh, float u, float v) {
  const WrapAxis ax = wrap_axis(u, sw), ay = wrap_axis(v, sh);
  const size_t r0 = (size_t)ay.i0 * (size_t)sw, r1 = (size_t)ay.i1 * (size_t)sw;
  const float t00 = load_channel<FORMAT, CH>(src, r0 + ax.i0), t10 = load_channel<FORMAT, CH>(src, r0 + ax.i1);
  const float t01 = load_channel<FORMAT, CH>(src, r1 + ax.i0), t11 = load_channel<FORMAT, CH>(src, r1 + ax.i1);
  return lerp_f(lerp_f(t00, t10, ax.f), lerp_f(t01, t11, ax.f), ay.f);
}

// ---- steps 7-9: the lens (lens.slang) -------------------------------------------------------------------------------------------------------
OXC_DEV void pcg3d16(uint32_t& x, uint32_t& y, uint32_t& z) {
  x = x * 12829u + 47989u, y = y * 12829u + 47989u, z = z * 12829u + 47989u;
  x += y * z, y += z * x, z += x * y;
  x += y * z, y += z * x, z += x * y;
  x >>= 16, y >>= 16, z >>= 16;
}
OXC_DEV float film_grain(uint32_t px, uint32_t py, const TonemapArgs& a) {
  uint32_t rx = px / a.grain_divisor, ry = py / a.grain_divisor, rz = a.grain_seed;
  pcg3d16(rx, ry, rz);
  const float fine_x = (float)rx * (1.0f / 65536.0f) - 0.5f, fine_y = (float)ry * (1.0f / 65536.0f) - 0.5f;  // exact
  const float P_x = (float)px / a.grain_scale + fine_x, P_y = (float)py / a.grain_scale + fine_y;
  const float F2 = 0.3660254037844386f, G2 = 0.21132486540518713f;  // the binary32 nearest (sqrt(3) - 1) / 2 and (3 - sqrt(3)) / 6
  const float u = (P_x + P_y) * F2;
  const float Pi_x = __builtin_rintf(P_x + u), Pi_y = __builtin_rintf(P_y + u);  // round half to even
  const float v = (Pi_x + Pi_y) * G2;
  const float f_x = P_x - (Pi_x - v), f_y = P_y - (Pi_y - v);
  const float length = __builtin_sqrtf(f_x * f_x + f_y * f_y);
  return 1.0f - 2.0f * exp2_rule((-length) * 3.0f);
}
}  // namespace

template <int TONEMAP, int FORMAT>
__global__ __launch_bounds__(256) void k_tonemap(TonemapArgs a) {
  const uint2 tp = tile_pixel();
  if (tp.x >= a.w || tp.y >= a.h) return;
  const size_t pix = (size_t)tp.y * a.w + tp.x;
  const Texel source = load_rgba<FORMAT>(a.src, pix);  // step 1
  V3 color = source.c;
  const float exposure = (a.flags & OXC_SCENE_HAS_EYE_ADAPTATION) ? a.exposure[1] : a.exposure_setting;  // step 2
  color = {color.x * exposure, color.y * exposure, color.z * exposure};
  if (a.flags & OXC_SCENE_HAS_BLOOM) {  // step 3
    const float u = ((float)tp.x + 0.5f) / (float)a.w, v = ((float)tp.y + 0.5f) / (float)a.h;
    const WrapAxis ax = wrap_axis(u, (int)a.bw), ay = wrap_axis(v, (int)a.bh);
    const size_t r0 = (size_t)ay.i0 * a.bw, r1 = (size_t)ay.i1 * a.bw;
    const V3 t00 = load_rgba<FORMAT>(a.bloom, r0 + ax.i0).c, t10 = load_rgba<FORMAT>(a.bloom, r0 + ax.i1).c;
    const V3 t01 = load_rgba<FORMAT>(a.bloom, r1 + ax.i0).c, t11 = load_rgba<FORMAT>(a.bloom, r1 + ax.i1).c;
    color.x = color.x + lerp_f(lerp_f(t00.x, t10.x, ax.f), lerp_f(t01.x, t11.x, ax.f), ay.f) * a.bloom_intensity;
    color.y = color.y + lerp_f(lerp_f(t00.y, t10.y, ax.f), lerp_f(t01.y, t11.y, ax.f), ay.f) * a.bloom_intensity;
    color.z = color.z + lerp_f(lerp_f(t00.z, t10.z, ax.f), lerp_f(t01.z, t11.z, ax.f), ay.f) * a.bloom_intensity;
  }
  if (TONEMAP == 1) color = aces_fitted(color);  // step 4
  if (TONEMAP == 2) color = agx_ds(color, a.k);
  if (TONEMAP == 3) color = gt7(color, a.k);
  const int cx = (int)(a.w / 2u), cy = (int)(a.h / 2u);
  const int dx = (int)tp.x - cx, dy = (int)tp.y - cy;
  if (a.flags & OXC_SCENE_HAS_CHROMATIC_ABERRATION) {  // step 7: re-sampled from the source, replaces the colour
    const float rcp_x = 1.0f / (float)(2 * cx), rcp_y = 1.0f / (float)(2 * cy);
    const float fdx = (float)dx, fdy = (float)dy, fcx = (float)cx, fcy = (float)cy;
    color.x = tap_channel<FORMAT, 0>(a.src, (int)a.w, (int)a.h, ((fdx * a.k.red_mag + fcx) + 0.5f) * rcp_x, ((fdy * a.k.red_mag + fcy) + 0.5f) * rcp_y);
    color.y = tap_channel<FORMAT, 1>(a.src, (int)a.w, (int)a.h, ((fdx * a.k.green_mag + fcx) + 0.5f) * rcp_x, ((fdy * a.k.green_mag + fcy) + 0.5f) * rcp_y);
    color.z = tap_channel<FORMAT, 2>(a.src, (int)a.w, (int)a.h, (float)tp.x * rcp_x, (float)tp.y * rcp_y);
  }
  if (a.flags & OXC_SCENE_HAS_VIGNETTE) {  // step 8
    const float pi_over_4 = 3.1415926535897932384626433832795f * 0.25f;
    float mx = cos_turn_rule((((float)abs(dx) / (float)cx) * a.vignette_amount) * pi_over_4);
    float my = cos_turn_rule((((float)abs(dy) / (float)cy) * a.vignette_amount) * pi_over_4);
    mx = mx * mx, my = my * my;
    mx = mx * mx, my = my * my;
    const float factor = clamp01(mx * my);
    color = {color.x * factor, color.y * factor, color.z * factor};
  }
  if (a.flags & OXC_SCENE_HAS_FILM_GRAIN) {  // step 9
    const float grain = film_grain(tp.x, tp.y, a);
    color.x = color.x + (grain * fminf(color.x, 1.0f - color.x)) * a.grain_amount;
    color.y = color.y + (grain * fminf(color.y, 1.0f - color.y)) * a.grain_amount;
    color.z = color.z + (grain * fminf(color.z, 1.0f - color.z)) * a.grain_amount;
  }
  const float alpha = (a.flags & OXC_SCENE_TRANSPARENT_BACKGROUND) ? source.a : 1.0f;  // step 10
  uint32_t r, g, b;  // step 11
  if (a.output_format == 2u) {
    r = pack_unorm(color.x), g = pack_unorm(color.y), b = pack_unorm(color.z);
  } else {
    r = pack_unorm(srgb_encode(color.x)), g = pack_unorm(srgb_encode(color.y)), b = pack_unorm(srgb_encode(color.z));
  }
  const uint32_t lo = a.output_format == 1u ? b : r, hi = a.output_format == 1u ? r : b;
  a.dst[pix] = lo | (g << 8) | (hi << 16) | (pack_unorm(alpha) << 24);
}

template <int TONEMAP>
static void launch_tonemap_format(const TonemapArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  if (a.format == 0u)
    hipLaunchKernelGGL((k_tonemap<TONEMAP, 0>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((k_tonemap<TONEMAP, 1>), grid, dim3(256), 0, s, a);
}

void launch_tonemap(const TonemapArgs& a, hipStream_t s) {
  switch (a.tonemap_type) {
    case 0: launch_tonemap_format<0>(a, s); break;
    case 1: launch_tonemap_format<1>(a, s); break;
    case 2: launch_tonemap_format<2>(a, s); break;
    default: launch_tonemap_format<3>(a, s); break;
  }
}

}  // namespace oxc
