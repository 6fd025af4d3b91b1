// oxcull_atmosphere.hip -- the four sky LUTs of the atmosphere path (gfx950): the constructor-time pair of RendererInstance.cpp:136-251
// (passes/sky_transmittance.slang, passes/sky_multiscattering.slang) and RendererInstance::draw_atmosphere (Passes/PBR.cpp:9-141:
// passes/sky_view.slang, passes/sky_aerial_perspective.slang), all through sky.slang.  Rules: include/oxcull.h, oxc_generate_sky_luts and
// oxc_draw_atmosphere; design: DESIGN.md section 21.
//
//   k_sky_transmittance   one texel per lane, blocks of one wave.  The 1000-step chain of a texel is serial (ray_pos and optical_depth are
//                         running sums), so a texel cannot be split across lanes without changing the order of its additions.
//   k_sky_multiscatter    one wave per texel, one lane per hemisphere direction, four texels per block.  A lane integrates its direction;
//                         the six per-direction sums go through LDS and lane c of 0 .. 2 adds channel c in ascending direction order, the
//                         order of the Slang's loop.
//   k_sky_view            one texel per lane, blocks of one wave; every texel runs 48 steps.
//   k_sky_aerial          a one-wave block holds 64 texels of ONE slice z (2 (z + 1) steps each), so the step count never diverges inside
//                         a wave; the blocks run from the highest z, the longest, down.  Two launches and not one grid with the sky view:
//                         the fused kernel spilled four SGPRs.
//   k_sky_ibl             the sky cubemap of oxc_generate_sky_ibl (passes/sky_ibl.slang): one wave per cube texel, one
//                         lane per sample, four texels per block; lane 0 adds the 64 samples in ascending order and stores the texel.
//
// integrate<> is sky.slang's integrate_single_scattered_luminance, its three constexpr switches template parameters; step<> is the body of
// its loop.  Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and
// sqrt are the IEEE ones, exp / pow / cos are the closed binary64 rules of oxcull_pixel_device.hpp, which also holds what the atmosphere branch
// of apply_pbr (oxcull_pbr_apply.hip) shares with this file: intersect, the clamp bilinear, the transmittance and the sky-view uv mappings.
#include <hip/hip_runtime.h>

#include <cmath>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

// ---- the host constants (the header's list) ----------------------------------------------------------------------------------------------------
void atmosphere_constants(const oxc_atmosphere& A, const float* camera_y, AtmosphereConstants& k) {
  const double ar = A.atmos_radius, pr = A.planet_radius, g = A.mie_asymmetry;
  k.h_atmos = (float)std::sqrt(std::fmax(0.0, ar * ar - pr * pr));
  // henyey_greenstein_draine_phase (common/math.slang:64-68): the argument in binary64, rounded to binary32, then the exp rule
  k.g_hg = exp_rule((float)(-((double)0.0990567f / (g - (double)1.67154f))));
  k.g_d = exp_rule((float)(-((double)2.20679f / (g + (double)3.91029f)) - (double)0.428934f));
  k.alpha = exp_rule((float)((double)3.62489f - ((double)8.29288f / (g + (double)5.52825f))));
  k.w_d = exp_rule((float)(-((double)0.599085f / (g - (double)0.641583f)) - (double)0.665888f));
  k.eye_altitude = k.beta = k.zenith_horizon_angle = 0.0f;
  if (!camera_y) return;
  // Atmosphere::get_eye_pos (scene.slang:229-233), then uv_to_sky_view_lut_params' texel-independent head (sky.slang:75-77)
  const double min_altitude = pr + (double)0.001f;
  k.eye_altitude = (float)std::fmax((double)*camera_y * (double)0.01f + min_altitude, min_altitude);
  const double h = k.eye_altitude;
  const double horizon = std::sqrt(std::fmax(0.0, h * h - pr * pr));
  const double beta = std::acos(horizon / h);
  k.beta = (float)beta;
  k.zenith_horizon_angle = (float)(0x1.921fb54442d18p+1 - beta);
}

namespace {
constexpr float kPi = 3.1415926535897932384626433832795f, kTau = 6.283185307179586476925286766559f;
constexpr float kPlanetRadiusOffset = 0.001f;
constexpr float kHalfMax = 65504.0f, kHalfMinNormal = 6.103515625e-5f;
constexpr float kInv4Pi = 1.0f / (4.0f * kPi), kRayleighK = 3.0f / (16.0f * kPi);

OXC_DEV float dotv(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
OXC_DEV float lengthv(const V3& a) { return __builtin_sqrtf(dotv(a, a)); }
OXC_DEV V3 along(const V3& o, float t, const V3& d) { return {o.x + t * d.x, o.y + t * d.y, o.z + t * d.z}; }  // o + t * d

// MediumScattering (sky.slang:119-150); mie_extinction is one float for the three channels
struct Medium {
  V3 rayleigh, mie, scattering, extinction;
};
OXC_DEV Medium medium_at(const oxc_atmosphere& A, float altitude) {
  const float rd = exp_rule(-altitude / A.rayleigh_density), md = exp_rule(-altitude / A.mie_density);
  const float od = fmaxf(0.0f, 1.0f - __builtin_fabsf(altitude - A.ozone_height) / A.ozone_thickness);
  Medium m;
  m.rayleigh = {A.rayleigh_scatter[0] * rd, A.rayleigh_scatter[1] * rd, A.rayleigh_scatter[2] * rd};
  m.mie = {A.mie_scatter[0] * md, A.mie_scatter[1] * md, A.mie_scatter[2] * md};
  const float me = A.mie_extinction * md;
  const V3 oz = {A.ozone_absorption[0] * od, A.ozone_absorption[1] * od, A.ozone_absorption[2] * od};
  m.scattering = {m.rayleigh.x + m.mie.x, m.rayleigh.y + m.mie.y, m.rayleigh.z + m.mie.z};
  m.extinction = {(m.rayleigh.x + me) + oz.x, (m.rayleigh.y + me) + oz.y, (m.rayleigh.z + me) + oz.z};
  return m;
}

// the transmittance sample of step 3 at (h, mu)
OXC_DEV V3 sun_transmittance_at(const SkyLutInputs& in, float h, float mu) {
  const oxc_atmosphere& A = in.atm;
  return transmittance_sample(in.transmittance, A.transmittance_lut_size[0], A.transmittance_lut_size[1], A.planet_radius, A.atmos_radius, in.k.h_atmos, h, mu);
}

// com::draine_phase (common/math.slang:58-62)
OXC_DEV float draine_phase(float alpha, float g, float c) {
  const float first = (1.0f - g * g) / pow_rule((1.0f + g * g) - (2.0f * g) * c, 1.5f);
  const float second = (1.0f + (alpha * c) * c) / (1.0f + (alpha * (1.0f / 3.0f)) * (1.0f + (2.0f * g) * g));
  return (kInv4Pi * first) * second;
}

struct Luminance {
  V3 luminance, multiscattering_as_1, transmittance;
};

// The body of the loop of integrate_single_scattered_luminance (sky.slang:206-238) at ray parameter `shift`, `step_length` after the last one
template <bool MS>
OXC_DEV void step(const SkyLutInputs& in, const V3& eye, const V3& dir, const V3& sun, float sun_intensity, float rayleigh_phase, float mie_phase, float shift,
                  float step_length, Luminance& r) {
  const oxc_atmosphere& A = in.atm;
  const V3 pos = along(eye, shift, dir);
  const float h = lengthv(pos), altitude = h - A.planet_radius;
  const Medium m = medium_at(A, altitude);
  const V3 up = {pos.x / h, pos.y / h, pos.z / h};
  const float sun_theta = dotv(sun, up);
  const V3 st = sun_transmittance_at(in, h, sun_theta);
  V3 ms = {0.0f, 0.0f, 0.0f};
  if (MS) {  // multiscattering_params_to_lut_uv (sky.slang:31-37)
    const float fw = (float)A.multiscattering_lut_size[0], fh = (float)A.multiscattering_lut_size[1];
    const float u = fminf(fmaxf(sun_theta * 0.5f + 0.5f, 0.0f), 1.0f), v = fminf(fmaxf(altitude / (A.atmos_radius - A.planet_radius), 0.0f), 1.0f);
    ms = sample_rgb(in.multiscatter, A.multiscattering_lut_size[0], A.multiscattering_lut_size[1], (u + 0.5f / fw) * (fw / (fw + 1.0f)),
                    (v + 0.5f / fh) * (fh / (fh + 1.0f)));
  }
  const V3 below = {pos.x - kPlanetRadiusOffset * up.x, pos.y - kPlanetRadiusOffset * up.y, pos.z - kPlanetRadiusOffset * up.z};
  const float earth_shadow = intersect_nearest(below, sun, A.planet_radius).has ? 0.0f : 1.0f;
  const float phase[3] = {m.mie.x * mie_phase + m.rayleigh.x * rayleigh_phase, m.mie.y * mie_phase + m.rayleigh.y * rayleigh_phase,
                          m.mie.z * mie_phase + m.rayleigh.z * rayleigh_phase};
  const float stc[3] = {st.x, st.y, st.z}, msc[3] = {ms.x, ms.y, ms.z}, sc[3] = {m.scattering.x, m.scattering.y, m.scattering.z};
  const float ex[3] = {m.extinction.x, m.extinction.y, m.extinction.z};
  float* lum[3] = {&r.luminance.x, &r.luminance.y, &r.luminance.z};
  float* as1[3] = {&r.multiscattering_as_1.x, &r.multiscattering_as_1.y, &r.multiscattering_as_1.z};
  float* tr[3] = {&r.transmittance.x, &r.transmittance.y, &r.transmittance.z};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float sun_luminance = (earth_shadow * stc[c]) * phase[c] + msc[c] * sc[c];
    const float step_transmittance = exp_rule(-step_length * ex[c]);
    const float integral = (sun_luminance - sun_luminance * step_transmittance) / ex[c];
    const float ms_integral = (sc[c] - sc[c] * step_transmittance) / ex[c];
    *lum[c] += sun_intensity * (integral * *tr[c]);
    *as1[c] += ms_integral * *tr[c];
    *tr[c] *= step_transmittance;
  }
}

// integrate_single_scattered_luminance (sky.slang:169-256).  TMAX false is the Slang's info.t_max == -1.0 (the default the multiscattering
// and the sky-view pass leave): the integration length comes from the intersections.  TMAX true is the aerial pass, whose t_max is
// max(0, ..) or a NaN and so never -1.0.
template <bool PLANET, bool MS, bool TMAX>
OXC_DEV Luminance integrate(const SkyLutInputs& in, const V3& eye, const V3& dir, const V3& sun, float sun_intensity, float step_count, float t_max) {
  const oxc_atmosphere& A = in.atm;
  Luminance r = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}};
  if (dotv(eye, eye) <= A.planet_radius * A.planet_radius) return r;
  const Hit planet = intersect_nearest(eye, dir, A.planet_radius);
  float integration_length = t_max;
  if (!TMAX) {
    const Hit atmos = intersect_nearest(eye, dir, A.atmos_radius);
    if (!atmos.has) return r;
    integration_length = planet.has ? fmaxf(0.0f, planet.value) : atmos.value;
  }
  const float cos_theta = dotv(sun, dir);
  const float rayleigh_phase = kRayleighK * (1.0f + cos_theta * cos_theta);
  const float hg = draine_phase(0.0f, in.k.g_hg, cos_theta), dr = draine_phase(in.k.alpha, in.k.g_d, cos_theta);
  const float mie_phase = lerp_f(hg, dr, in.k.w_d);
  float old_ray_shift = 0.0f;
#pragma unroll 1
  for (float s = 0.0f; s < step_count; s += 1.0f) {
    const float new_ray_shift = (integration_length * (s + 0.3f)) / step_count;
    step<MS>(in, eye, dir, sun, sun_intensity, rayleigh_phase, mie_phase, new_ray_shift, new_ray_shift - old_ray_shift, r);
    old_ray_shift = new_ray_shift;
  }
  if (PLANET && planet.has && integration_length == planet.value) {  // the light the ground bounces back (sky.slang:242-253)
    const V3 pos = along(eye, integration_length, dir);
    const float h = lengthv(pos);
    const V3 up = {pos.x / h, pos.y / h, pos.z / h};
    const float sun_theta = dotv(sun, up);
    const float nol = saturate_f(dotv(normalize3(sun), normalize3(up)));
    const V3 st = sun_transmittance_at(in, h, sun_theta);
    r.luminance.x += sun_intensity * ((((st.x * r.transmittance.x) * nol) * A.terrain_albedo[0]) / kPi);
    r.luminance.y += sun_intensity * ((((st.y * r.transmittance.y) * nol) * A.terrain_albedo[1]) / kPi);
    r.luminance.z += sun_intensity * ((((st.z * r.transmittance.z) * nol) * A.terrain_albedo[2]) / kPi);
  }
  return r;
}

// move_to_top_atmosphere (sky.slang:104-117)
OXC_DEV bool move_to_top_atmosphere(V3& pos, const V3& dir, float atmos_radius) {
  const float h = lengthv(pos);
  if (h > atmos_radius) {
    const Hit top = intersect_nearest(pos, dir, atmos_radius);
    if (!top.has) return false;
    const V3 up = {pos.x / h, pos.y / h, pos.z / h};
    pos = {(pos.x + dir.x * top.value) + up.x * -kPlanetRadiusOffset, (pos.y + dir.y * top.value) + up.y * -kPlanetRadiusOffset,
           (pos.z + dir.z * top.value) + up.z * -kPlanetRadiusOffset};
  }
  return true;
}

OXC_DEV void store_half4(uint2* dst, size_t i, float x, float y, float z, float w) {
  dst[i] = make_uint2(channel_half(x) | (channel_half(y) << 16), channel_half(z) | (channel_half(w) << 16));
}

// sky_view.slang for texel (x, y)
OXC_DEV void sky_view_texel(const AtmosphereArgs& a, uint32_t x, uint32_t y) {
  const oxc_atmosphere& A = a.in.atm;
  const uint32_t w = A.sky_view_lut_size[0], hgt = A.sky_view_lut_size[1];
  const float fw = (float)w, fh = (float)hgt;
  const size_t at = (size_t)y * w + x;
  V3 eye = {0.0f, a.in.k.eye_altitude, 0.0f};
  const float h = a.in.k.eye_altitude;  // length(eye_pos): the square root of a square
  // uv_to_sky_view_lut_params (sky.slang:69-102)
  const float u = (((float)x + 0.5f) / fw - 0.5f / fw) * (fw / (fw - 1.0f)), v = (((float)y + 0.5f) / fh - 0.5f / fh) * (fh / (fh - 1.0f));
  const float zha = a.in.k.zenith_horizon_angle, beta = a.in.k.beta;
  float view_zenith_angle;
  if (v < 0.5f) {
    float coord = v * 2.0f;
    coord = 1.0f - coord;
    coord *= coord;
    coord = 1.0f - coord;
    view_zenith_angle = zha * coord;
  } else {
    float coord = v * 2.0f - 1.0f;
    coord *= coord;
    view_zenith_angle = zha + beta * coord;
  }
  const float longitude = u * kTau;
  const float cz = cos_turn_rule(view_zenith_angle), sz = safe_sqrt(1.0f - cz * cz) * (view_zenith_angle > 0.0f ? 1.0f : -1.0f);
  const float cl = cos_turn_rule(longitude), sl = safe_sqrt(1.0f - cl * cl) * (longitude <= kPi ? 1.0f : -1.0f);
  const V3 dir = {sz * cl, cz, sz * sl};
  if (!move_to_top_atmosphere(eye, dir, A.atmos_radius)) {
    store_half4(a.sky_view, at, 0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const V3 up = {eye.x / h, eye.y / h, eye.z / h};
  const float szc = dotv({a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]}, up);
  const V3 sun = normalize3({safe_sqrt(1.0f - szc * szc), szc, 0.0f});
  const Luminance r = integrate<false, false, false>(a.in, eye, dir, sun, a.sun_intensity, 48.0f, -1.0f);
  const auto clean = [](float c) {  // com::sanitize(max(c, 0.0)): a NaN is already 0 after the max
    const float m = fmaxf(c, 0.0f);
    return m < __builtin_inff() ? m : 0.0f;
  };
  const float lx = clean(r.luminance.x), ly = clean(r.luminance.y), lz = clean(r.luminance.z);
  const float mult = fminf(fmaxf(fmaxf(lx, fmaxf(ly, lz)), kHalfMinNormal), kHalfMax);
  store_half4(a.sky_view, at, lx / mult, ly / mult, lz / mult, mult);
}

// sky_aerial_perspective.slang for texel (x, y, z)
OXC_DEV void aerial_texel(const AtmosphereArgs& a, uint32_t x, uint32_t y, uint32_t z) {
  const oxc_atmosphere& A = a.in.atm;
  const uint32_t w = A.aerial_perspective_lut_size[0], hgt = A.aerial_perspective_lut_size[1], dep = A.aerial_perspective_lut_size[2];
  const size_t at = ((size_t)z * hgt + y) * w + x;
  const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)hgt;
  V3 world;
  unproject(a.inv_projection_view, u, v, 1.0f, world.x, world.y, world.z);
  const V3 dir = normalize3({world.x - a.camera_position[0], world.y - a.camera_position[1], world.z - a.camera_position[2]});
  V3 eye = {0.0f, a.in.k.eye_altitude, 0.0f};
  float slice = ((float)z + 0.5f) * (1.0f / (float)dep);
  slice *= slice;
  slice *= (float)dep;
  const float per_slice_depth = (float)((int)w / (int)dep);  // the Slang divides two i32
  float t_max_max = slice * per_slice_depth;
  if (a.in.k.eye_altitude >= A.atmos_radius) {
    const V3 prev = eye;
    if (!move_to_top_atmosphere(eye, dir, A.atmos_radius)) {
      store_half4(a.aerial, at, 0.0f, 0.0f, 0.0f, 0.0f);
      return;
    }
    const float length_to_atmosphere = lengthv({prev.x - eye.x, prev.y - eye.y, prev.z - eye.z});
    if (t_max_max < length_to_atmosphere) {
      store_half4(a.aerial, at, 0.0f, 0.0f, 0.0f, 0.0f);
      return;
    }
    t_max_max = fmaxf(0.0f, t_max_max - length_to_atmosphere);
  }
  const float step_count = fmaxf(1.0f, ((float)z + 1.0f) * 2.0f);
  const Luminance r = integrate<false, false, true>(a.in, eye, dir, {a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]}, a.sun_intensity, step_count, t_max_max);
  const float third = 1.0f / 3.0f;
  store_half4(a.aerial, at, r.luminance.x, r.luminance.y, r.luminance.z, (r.transmittance.x * third + r.transmittance.y * third) + r.transmittance.z * third);
}
// ---- the sky cubemap (passes/sky_ibl.slang; the header's steps 11 - 15) -----------------------------------------------------------------------
OXC_DEV float frac_f(float x) { return x - floorf(x); }
OXC_DEV float finite_or_zero(float x) { return __builtin_fabsf(x) < __builtin_inff() ? x : 0.0f; }  // com::sanitize, one component

// CUBE_MAP_FACE_ROTATION (sky_ibl.slang:21-30), the nine scalars in the constructor's order: row r is elements 3 r .. 3 r + 2
__constant__ const float kCubeFace[6][9] = {{+0, +0, -1, +0, -1, +0, -1, +0, +0}, {+0, +0, +1, +0, -1, +0, +1, +0, +0}, {+1, +0, +0, +0, +0, -1, +0, +1, +0},
                                            {+1, +0, +0, +0, +0, +1, +0, -1, +0}, {+1, +0, +0, +0, -1, +0, +0, +0, -1}, {-1, +0, +0, +0, -1, +0, +0, +0, +1}};

// get_atmosphere_illuminance_along_ray (sky.slang:296-322), sanitized
OXC_DEV V3 sky_illuminance(const SkyIblArgs& a, const V3& eye, const V3& dir) {
  const oxc_atmosphere& A = a.in.atm;
  const float height = lengthv(eye);
  const V3 up = {eye.x / height, eye.y / height, eye.z / height};
  const float view_zenith_cos_angle = dotv(dir, up);
  const V3 side_raw = crossv(up, dir);
  const V3 side = lengthv(side_raw) > 1e-5f ? normalize3(side_raw) : V3{1.0f, 0.0f, 0.0f};
  const V3 forward = normalize3(crossv(side, up));
  const V3 sun = normalize3({a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]});
  float lx = dotv(sun, forward), ly = dotv(sun, side);
  const float len_sq = lx * lx + ly * ly;
  const float inv_len = 1.0f / __builtin_sqrtf(len_sq);
  const bool keep = len_sq > 1e-20f;  // false for a NaN
  lx = keep ? lx * inv_len : 1.0f;
  ly = keep ? ly * inv_len : 0.0f;
  const bool intersect_planet = intersect_nearest(eye, dir, A.planet_radius).has;
  float u, v;
  sky_view_lut_uv(a.in.k.zenith_horizon_angle, a.in.k.beta, A.sky_view_lut_size[0], A.sky_view_lut_size[1], intersect_planet, view_zenith_cos_angle, lx, ly, u, v);
  const Texel t = sample_rgba(a.sky_view, A.sky_view_lut_size[0], A.sky_view_lut_size[1], u, v);
  return {finite_or_zero(t.c.x * t.a), finite_or_zero(t.c.y * t.a), finite_or_zero(t.c.z * t.a)};
}
}  // namespace

// sky_transmittance.slang
__global__ __launch_bounds__(64) void k_sky_transmittance(SkyLutArgs a) {
  const oxc_atmosphere& A = a.in.atm;
  const uint32_t w = A.transmittance_lut_size[0], hgt = A.transmittance_lut_size[1];
  const uint32_t p = blockIdx.x * 64u + threadIdx.x;
  if (p >= w * hgt) return;
  const uint32_t x = p % w, y = p / w;
  const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)hgt;
  const float h = a.in.k.h_atmos, pr = A.planet_radius;
  const float rho = h * v;
  const float lut_x = __builtin_sqrtf(rho * rho + pr * pr);
  const float d_min = A.atmos_radius - lut_x, d_max = rho + h;
  const float d = d_min + u * (d_max - d_min);
  float lut_y = d == 0.0f ? 1.0f : ((h * h - rho * rho) - d * d) / ((2.0f * lut_x) * d);
  lut_y = fminf(fmaxf(lut_y, -1.0f), 1.0f);
  const V3 sun = {0.0f, __builtin_sqrtf(1.0f - lut_y * lut_y), lut_y};
  V3 pos = {0.0f, 0.0f, lut_x};
  const float distance_per_step = intersect_nearest(pos, sun, A.atmos_radius).value / 1000.0f;
  V3 optical_depth = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (float i = 0.0f; i < 1000.0f; i += 1.0f) {
    pos = {pos.x + sun.x * distance_per_step, pos.y + sun.y * distance_per_step, pos.z + sun.z * distance_per_step};
    const Medium m = medium_at(A, lengthv(pos) - pr);
    optical_depth = {optical_depth.x + m.extinction.x * distance_per_step, optical_depth.y + m.extinction.y * distance_per_step,
                     optical_depth.z + m.extinction.z * distance_per_step};
  }
  store_half4(a.transmittance, p, exp_rule(-optical_depth.x), exp_rule(-optical_depth.y), exp_rule(-optical_depth.z), 1.0f);
}

// sky_multiscattering.slang
__global__ __launch_bounds__(256) void k_sky_multiscatter(SkyLutArgs a) {
  __shared__ float part[4][6][64];
  const oxc_atmosphere& A = a.in.atm;
  const uint32_t w = A.multiscattering_lut_size[0], hgt = A.multiscattering_lut_size[1];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t p = blockIdx.x * 4u + wave;
  const bool live = p < w * hgt;  // wave-uniform
  const uint32_t x = p % w, y = p / w;
  if (live) {
    const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)hgt;
    const float altitude = (A.planet_radius + v * (A.atmos_radius - A.planet_radius)) + kPlanetRadiusOffset;
    const float sun_cos_theta = u * 2.0f - 1.0f;
    const V3 sun = {0.0f, sun_cos_theta, safe_sqrt(1.0f - sun_cos_theta * sun_cos_theta)};
    const V3 dir = {a.hemisphere[lane * 3u], a.hemisphere[lane * 3u + 1u], a.hemisphere[lane * 3u + 2u]};
    // AtmosphereIntegrateInfo's defaults: sun_intensity 10.0, t_max -1.0; step_count 32
    const Luminance r = integrate<true, false, false>(a.in, {0.0f, altitude, 0.0f}, dir, sun, 10.0f, 32.0f, -1.0f);
    part[wave][0][lane] = r.luminance.x, part[wave][1][lane] = r.luminance.y, part[wave][2][lane] = r.luminance.z;
    part[wave][3][lane] = r.multiscattering_as_1.x, part[wave][4][lane] = r.multiscattering_as_1.y, part[wave][5][lane] = r.multiscattering_as_1.z;
  }
  __syncthreads();
  if (!live || lane > 3u) return;
  unsigned short* out = reinterpret_cast<unsigned short*>(a.multiscatter) + (size_t)p * 4u;
  if (lane == 3u) {
    out[3] = 0x3C00u;  // 1.0
    return;
  }
  float luminance = 0.0f, as1 = 0.0f;
#pragma unroll 1
  for (int i = 0; i < 64; i++) {
    as1 += part[wave][3 + lane][i];
    luminance += part[wave][lane][i];
  }
  const float sphere_solid_angle = 4.0f * kPi, isotropic_phase = 1.0f / sphere_solid_angle, inv_sample_count = 1.0f / 64.0f;
  luminance *= sphere_solid_angle * inv_sample_count;
  as1 *= inv_sample_count;
  const float scattered = luminance * isotropic_phase, f_ms = 1.0f / (1.0f - as1);
  out[lane] = (unsigned short)channel_half(scattered * f_ms);
}

// sky_view.slang: 64 texels per one-wave block, 48 steps each
__global__ __launch_bounds__(64) void k_sky_view(AtmosphereArgs a) {
  const uint32_t p = blockIdx.x * 64u + threadIdx.x, w = a.in.atm.sky_view_lut_size[0];
  if (p < w * a.in.atm.sky_view_lut_size[1]) sky_view_texel(a, p % w, p / w);
}

// sky_aerial_perspective.slang: a one-wave block holds 64 texels of one slice; the slices run from the highest z, the longest, down
__global__ __launch_bounds__(64) void k_sky_aerial(AtmosphereArgs a) {
  const uint32_t* size = a.in.atm.aerial_perspective_lut_size;
  const uint32_t z = size[2] - 1u - blockIdx.x / a.slice_blocks;
  const uint32_t p = (blockIdx.x % a.slice_blocks) * 64u + threadIdx.x;
  if (p < size[0] * size[1]) aerial_texel(a, p % size[0], p / size[0], z);
}

// sky_ibl.slang: one wave per cube texel, one lane per sample of its 64, four texels per block.  Every lane evaluates the texel's frame
// (a few dozen operations, the same in all 64 lanes) and its own sample; the three sums go through LDS and lane 0 adds them in ascending
// sample order, then handles the sun term, the history and the store.
__global__ __launch_bounds__(256) void k_sky_ibl(SkyIblArgs a) {
  __shared__ float part[4][3][64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t p = blockIdx.x * 4u + wave;
  const bool live = p < a.texels;  // wave-uniform
  const V3 eye = {0.0f, a.in.k.eye_altitude, 0.0f};
  V3 output_dir = {0.0f, 0.0f, 0.0f};
  Texel history = {{0.0f, 0.0f, 0.0f}, 0.0f};
  bool has_history = false;
  if (live) {
    const uint32_t cs = a.cube_size, face = p / (cs * cs), rem = p - face * (cs * cs), x = rem % cs, y = rem / cs;
    const float fcs = (float)cs;
    const float u = ((float)x + 0.5f) / fcs, v = ((float)y + 0.5f) / fcs;
    const V3 in = {u * 2.0f - 1.0f, v * 2.0f - 1.0f, -1.0f};
    const float* m = kCubeFace[face];
    output_dir = normalize3({(m[0] * in.x + m[1] * in.y) + m[2] * in.z, (m[3] * in.x + m[4] * in.y) + m[5] * in.z, (m[6] * in.x + m[7] * in.y) + m[8] * in.z});
    const V3 up = __builtin_fabsf(output_dir.y) < 0.999f ? V3{0.0f, 1.0f, 0.0f} : V3{1.0f, 0.0f, 0.0f};
    const V3 tangent = normalize3(crossv(up, output_dir));
    const V3 bitangent = crossv(output_dir, tangent);
    history = load_rgba<1>(a.cube, p);
    has_history = history.a > 0.0f && __builtin_fabsf(history.c.x) < __builtin_inff() && __builtin_fabsf(history.c.y) < __builtin_inff() &&
                  __builtin_fabsf(history.c.z) < __builtin_inff();
    // interleaved_gradient_noise(f32x2(pixel) + f32(face) * (37, 17))
    const float px = (float)x + (float)face * 37.0f, py = (float)y + (float)face * 17.0f;
    const float base_rotation = frac_f(52.9829189f * frac_f(px * 0.06711056f + py * 0.00583715f));
    const float rotation = has_history ? frac_f(base_rotation + (float)a.frame_index * 0.61803398875f) : base_rotation;
    // cosine_hemisphere_sample(lane, 64, rotation)
    const float u1 = ((float)lane + 0.5f) / 64.0f;
    const float u2 = frac_f((float)__builtin_bitreverse32(lane) * 2.3283064365386963e-10f + rotation);
    const float r = __builtin_sqrtf(u1), phi = kTau * u2;
    float cs_phi, sn_phi;
    cos_sin_angle_rule(phi, cs_phi, sn_phi);
    const float lx = r * cs_phi, ly = r * sn_phi, lz = __builtin_sqrtf(fmaxf(0.0f, 1.0f - u1));
    const V3 input_dir = normalize3({(lx * tangent.x + ly * bitangent.x) + lz * output_dir.x, (lx * tangent.y + ly * bitangent.y) + lz * output_dir.y,
                                     (lx * tangent.z + ly * bitangent.z) + lz * output_dir.z});
    const V3 sample = sky_illuminance(a, eye, input_dir);
    part[wave][0][lane] = sample.x, part[wave][1][lane] = sample.y, part[wave][2][lane] = sample.z;
  }
  __syncthreads();
  if (!live || lane != 0u) return;
  float sum[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (int i = 0; i < 64; i++) {
    sum[0] += part[wave][0][i];
    sum[1] += part[wave][1][i];
    sum[2] += part[wave][2][i];
  }
  const float sun_cos_zenith = (a.sun_dir[0] * 0.0f + a.sun_dir[1] * 1.0f) + a.sun_dir[2] * 0.0f;
  const V3 sun_color = sun_transmittance_at(a.in, eye.y, sun_cos_zenith);
  const float sun_facing = saturate_f(dotv(output_dir, {a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]}));
  const float sc[3] = {sun_color.x, sun_color.y, sun_color.z}, hist[3] = {history.c.x, history.c.y, history.c.z};
  float out[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float frame_estimate = sum[c] / 64.0f;
    const float sun_term = (((a.sun_ambient_strength * sc[c]) * a.sun_intensity) * sun_facing) / kPi;
    const float clean = finite_or_zero(frame_estimate + sun_term);
    const float positive = clean > 0.0f ? clean : 0.0f;  // the clamp as two selects: a negative zero becomes +0
    const float frame_result = positive < kHalfMax ? positive : kHalfMax;
    out[c] = has_history ? lerp_f(hist[c], frame_result, 0.02f) : frame_result;
  }
  store_half4(a.cube, p, out[0], out[1], out[2], 1.0f);
}

void launch_sky_luts(const SkyLutArgs& a, hipStream_t s) {
  const oxc_atmosphere& A = a.in.atm;
  hipLaunchKernelGGL(k_sky_transmittance, dim3((A.transmittance_lut_size[0] * A.transmittance_lut_size[1] + 63u) / 64u), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_sky_multiscatter, dim3((A.multiscattering_lut_size[0] * A.multiscattering_lut_size[1] + 3u) / 4u), dim3(256), 0, s, a);
}

void launch_atmosphere(AtmosphereArgs a, hipStream_t s) {
  const oxc_atmosphere& A = a.in.atm;
  a.slice_blocks = (A.aerial_perspective_lut_size[0] * A.aerial_perspective_lut_size[1] + 63u) / 64u;
  hipLaunchKernelGGL(k_sky_view, dim3((A.sky_view_lut_size[0] * A.sky_view_lut_size[1] + 63u) / 64u), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_sky_aerial, dim3(A.aerial_perspective_lut_size[2] * a.slice_blocks), dim3(64), 0, s, a);
}

void launch_sky_ibl(const SkyIblArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_sky_ibl, dim3((a.texels + 3u) / 4u), dim3(256), 0, s, a); }

}  // namespace oxc
