// oxcull_pbr_apply.hip -- the lit HDR image from the G-buffer and the shadow terms (gfx950): the no-atmosphere branch of
// RendererInstance::apply_pbr (Oxylus/src/Render/Passes/PBR.cpp:313-534, passes/pbr_apply_no_atmos.slang with pbr.slang) as one compute
// launch.  Rules: include/oxcull.h, oxc_apply_pbr; design and measurements: DESIGN.md section 16.
//
//   k_pbr_apply   one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block), as the other per-pixel passes.  The fixed
//                 part is eight image loads and one store; the light loop is the variable part.
//                 - The 256 results of the sRGB decode are filled once per block into LDS, one entry per thread: three pow off every pixel.
//                 - What a spot light does not owe to the pixel -- the two cosines (binary64 polynomials) and the normalised direction --
//                   is worked out once per block, one light per thread, in chunks of 256 lights (kLightChunk) into LDS; a pixel's loop reads
//                   it back with a wave-uniform index (a broadcast read).
//                 - A light's record is read through a const __restrict__ pointer with a wave-uniform index: scalar loads, no VGPRs.  The
//                   early-outs of a light (attenuation, intensity, NdotL) depend on the pixel: lane divergence, not branches around the load.
//                 - F0, alpha, alpha2, GGX_directional_albedo and the energy compensation do not depend on the light: BRDF recomputes them
//                   with the same operands for every light, here they are computed once per pixel.  Same operations, same bits.
//                 Threads outside the image and pixels that are done early (transparent empty, sky) stay for the block's barriers.
//   k_pbr_apply_atmosphere   the atmosphere branch (passes/pbr_apply.slang with sky.slang; oxc_apply_pbr_atmosphere): the
//                 same shape and, through the helpers both kernels call, the same decode, frame, surface terms, light loop and BRDF.  The
//                 sun's colour comes from the transmittance LUT per pixel, the ambient term from two face-local bilinear samples of the sky
//                 cube, a lit pixel adds the aerial-perspective LUT's in-scattering, and a sky pixel is the sky-view LUT plus the sun disc.
//                 The LUTs and the cube are read from global memory (L2), not staged; the binary64 acos / atan2 / exp sit in the sky arm.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and square
// root are the IEEE ones, pow / exp2 / cos are the closed forms in binary64.  The wave's FP16 denormal mode stays at its default (denormals
// kept: the normal and ambient-occlusion images hold denormal halves); the kernel must not call set_half_denorm_flush().
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr uint32_t kLightChunk = 256;  // lights staged per round: one per thread of the block
constexpr float kPi = 3.1415926535897932f;

// GPU::Light, scene.slang:272-283
struct GpuLight {
  float position[3];
  float intensity;
  float color[3];
  float range;
  float direction[3];
  float inner_cone_angle, outer_cone_angle;
  uint32_t kind;
  uint32_t pad[2];
};
static_assert(sizeof(GpuLight) == 64, "GPU::Light is 64 bytes");

// what a spot light does not owe to the pixel
struct SpotTerms {
  float cos_inner, cos_outer, dx, dy, dz;  // normalize(direction)
};

OXC_DEV float clamp_f(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// the cos rule of oxc_apply_pbr: binary64, two-constant reduction, the polynomials of cos_sin_turn, one rounding
__host__ OXC_DEV float cos_rule(float x) {
  const float ax = __builtin_fabsf(x);
  if (!(ax <= 0x1p+24f)) return __builtin_nanf("");  // non-finite or beyond 2^24
  const double a = (double)ax;
  const double q = __builtin_floor(a * 0x1.45f306dc9c883p-1 + 0.5);
  const double r = (a - q * 0x1.921fb54p+0) - q * 0x1.10b4611a62633p-30;
  const double z = r * r;
  const double ps = ((0x1.71de3a556c734p-19 * z + -0x1.a01a01a01a01ap-13) * z + 0x1.1111111111111p-7) * z + -0x1.5555555555555p-3;
  const double s = r + (r * z) * ps;
  const double pc = (((-0x1.27e4fb7789f5cp-22 * z + 0x1.a01a01a01a01ap-16) * z + -0x1.6c16c16c16c17p-10) * z + 0x1.5555555555555p-5) * z + -0x1.0000000000000p-1;
  const double c = 1.0 + z * pc;
  const uint32_t n = (uint32_t)(long long)q & 3u;
  const double v = n == 0u ? c : n == 1u ? -s : n == 2u ? -c : s;
  return (float)v;
}

// what BRDF (pbr.slang:61-87) takes from the pixel alone
struct Surface {
  V3 N, V;
  float albedo[3], F0[3], ec[3];  // ec: GGX_energy_compensation(NoV, alpha, F0)
  float metallic, NoV, alpha2;
};

// BRDF(V, N, l): diffuse and specular per channel
OXC_DEV void brdf(const Surface& s, const V3& l, float* diffuse, float* specular) {
  const V3 VL = {s.V.x + l.x, s.V.y + l.y, s.V.z + l.z};
  const V3 H = dot3v(VL, VL) > 1e-8f ? normalize3(VL) : s.N;
  const float NoL = saturate_f(dot3v(s.N, l));
  const float NoH = saturate_f(dot3v(s.N, H));
  const float LoH = saturate_f(dot3v(l, H));
  const float f = (NoH * s.alpha2 - NoH) * NoH + 1.0f;
  const float D = s.alpha2 / ((kPi * f) * f + 1e-7f);
  const float GGXV = NoL * __builtin_sqrtf((s.NoV * s.NoV) * (1.0f - s.alpha2) + s.alpha2);
  const float GGXL = s.NoV * __builtin_sqrtf((NoL * NoL) * (1.0f - s.alpha2) + s.alpha2);
  const float Vis = saturate_f(0.5f / ((GGXV + GGXL) + 1e-7f));
  const float p5 = pow_rule(saturate_f(1.0f - LoH), 5.0f);
  const float lambert = 1.0f / kPi;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float F = s.F0[c] + (1.0f - s.F0[c]) * p5;
    specular[c] = ((D * Vis) * F) * s.ec[c];
    diffuse[c] = (((1.0f - s.metallic) * (1.0f - F)) * s.albedo[c]) * lambert;
  }
}

// GGX_directional_albedo's nine float4 constants, pbr.slang:40-42
__constant__ const float kAlbedoFit[9][4] = {{0.1003f, 0.9345f, 1.0f, 1.0f},        {-0.6303f, -2.323f, -1.765f, 0.2281f}, {9.748f, 2.229f, 8.263f, 15.94f},
                                             {-2.038f, -3.748f, 11.53f, -55.83f},   {29.34f, 1.424f, 28.96f, 13.08f},      {-8.245f, -0.7684f, -7.507f, 41.26f},
                                             {-26.44f, 1.436f, -36.11f, 54.9f},     {19.99f, 0.2913f, 15.86f, 300.2f},     {-5.448f, 0.6286f, 33.37f, -285.1f}};
// what steps 2 - 4 of oxc_apply_pbr give a pixel
struct Pixel {
  Surface s;
  V3 world, smooth, R;
  float emission[3];
  float roughness, occlusion, NoL;
};

// steps 2 - 4 of oxc_apply_pbr: decode, position, frame
OXC_DEV void decode_and_frame(const PbrApplyArgs& a, const float* s_srgb, uint32_t px, uint32_t py, size_t pix, float depth, Pixel& p) {
  Surface& s = p.s;
  // 2. decode
  const uint32_t albedo_w = a.albedo[pix];
  const uint2 normal_w = a.normal[pix];
  const uint32_t emissive_w = a.emissive[pix], mro_w = a.mro[pix];
  const uint32_t ao_h = a.ao[pix];
  s.albedo[0] = s_srgb[albedo_w & 0xFFu], s.albedo[1] = s_srgb[(albedo_w >> 8) & 0xFFu], s.albedo[2] = s_srgb[(albedo_w >> 16) & 0xFFu];
  const V3 mapped = oct_to_vec3(normal_w.x);
  p.smooth = oct_to_vec3(normal_w.y);
  p.emission[0] = unpack_ufloat<6>(emissive_w & 0x7FFu), p.emission[1] = unpack_ufloat<6>((emissive_w >> 11) & 0x7FFu), p.emission[2] = unpack_ufloat<5>(emissive_w >> 22);
  s.metallic = clamp_f((float)(mro_w & 0xFFu) / 255.0f, 0.0f, 1.0f);
  p.roughness = clamp_f((float)((mro_w >> 8) & 0xFFu) / 255.0f, 0.045f, 1.0f);
  p.occlusion = ((float)((mro_w >> 16) & 0xFFu) / 255.0f) * dequantize_half(ao_h);
  // 3. position
  const float u = ((float)px + 0.5f) / a.fw, v = ((float)py + 0.5f) / a.fh;
  unproject(a.inv_pv, u, v, depth, p.world.x, p.world.y, p.world.z);
  // 4. frame
  s.V = normalize3({a.camera[0] - p.world.x, a.camera[1] - p.world.y, a.camera[2] - p.world.z});
  s.N = normalize3(mapped);
  const V3 nV = {-s.V.x, -s.V.y, -s.V.z};
  const float two_d = 2.0f * dot3v(s.N, nV);
  p.R = {nV.x - two_d * s.N.x, nV.y - two_d * s.N.y, nV.z - two_d * s.N.z};
  s.NoV = __builtin_fabsf(dot3v(s.N, s.V)) + 1e-5f;
  p.NoL = fmaxf(dot3v(s.N, {a.sun[0], a.sun[1], a.sun[2]}), 0.0f);
}

// step 7 and what step 8 takes from the pixel alone: alpha2, F0, the energy compensation; AB and spec_occlusion for the ambient term
OXC_DEV void surface_terms(Pixel& p, float& ABx, float& ABy, float& spec_occlusion) {
  Surface& s = p.s;
  const float alpha = fmaxf(p.roughness * p.roughness, 0.0025f);
  s.alpha2 = alpha * alpha;
  const float x = s.NoV, y = alpha, x2 = x * x, y2 = y * y;
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; k++)
    r[k] = (((((((kAlbedoFit[0][k] + kAlbedoFit[1][k] * x) + kAlbedoFit[2][k] * y) + (kAlbedoFit[3][k] * x) * y) + kAlbedoFit[4][k] * x2) + kAlbedoFit[5][k] * y2) +
             (kAlbedoFit[6][k] * x2) * y) +
            (kAlbedoFit[7][k] * x) * y2) +
           (kAlbedoFit[8][k] * x2) * y2;
  ABx = clamp_f(r[0] / r[2], 0.0f, 1.0f), ABy = clamp_f(r[1] / r[3], 0.0f, 1.0f);
  const float Ess = saturate_f(ABx + ABy);
  spec_occlusion = saturate_f((pow_rule(s.NoV + p.occlusion, exp2_rule(-16.0f * p.roughness - 1.0f)) - 1.0f) + p.occlusion);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    s.F0[c] = 0.04f + (s.albedo[c] - 0.04f) * s.metallic;
    s.ec[c] = 1.0f + (s.F0[c] * (1.0f - Ess)) / fmaxf(Ess, 1e-4f);
  }
}

// step 9 of oxc_apply_pbr, for the whole block (every thread comes here: the barriers): in chunks, a barrier, one light's pixel-independent
// terms per thread, a barrier, then every shading pixel walks the chunk.  n: the four outcome counts {kind, attenuation, NdotL, shaded}.
OXC_DEV void walk_lights(const PbrApplyArgs& a, SpotTerms* s_spot, uint32_t tid, bool shade, const Surface& s, const V3& world, float* total, uint32_t* n) {
  const GpuLight* __restrict__ lights = static_cast<const GpuLight*>(a.lights);
  for (uint32_t base = 0; base < a.light_count; base += kLightChunk) {
    if (base) __syncthreads();  // the previous chunk has been read
    const uint32_t mine = base + tid;
    if (mine < a.light_count && lights[mine].kind == 2u) {
      const GpuLight& l = lights[mine];
      const V3 d = normalize3({l.direction[0], l.direction[1], l.direction[2]});
      s_spot[tid] = {cos_rule(l.inner_cone_angle), cos_rule(l.outer_cone_angle), d.x, d.y, d.z};
    }
    __syncthreads();
    if (shade) {
      const uint32_t end = min(a.light_count - base, kLightChunk);
#pragma unroll 1
      for (uint32_t j = 0; j < end; j++) {
        const GpuLight& l = lights[base + j];
        const uint32_t kind = l.kind;
        if (kind != 1u && kind != 2u) {
          n[0]++;
          continue;
        }
        const V3 lv = {l.position[0] - world.x, l.position[1] - world.y, l.position[2] - world.z};
        const float dist = len3(lv.x, lv.y, lv.z);
        const V3 Ll = {lv.x / dist, lv.y / dist, lv.z / dist};
        const float range = l.range, d2 = dist * dist + 0.1f;
        float attenuation;
        if (range <= 0.0f) {
          attenuation = 1.0f / d2;
        } else {
          float win = dist / range;
          win = ((win * win) * win) * win;
          win = fmaxf(0.0f, 1.0f - win);
          win = win * win;
          attenuation = win / d2;
        }
        if (kind == 2u) {
          const SpotTerms sp = s_spot[j];
          const float cos_angle = dot3v({-Ll.x, -Ll.y, -Ll.z}, {sp.dx, sp.dy, sp.dz});
          const float t = saturate_f((cos_angle - sp.cos_outer) / (sp.cos_inner - sp.cos_outer));
          attenuation = attenuation * ((t * t) * (3.0f - 2.0f * t));
        }
        const float intensity = l.intensity;
        if (attenuation <= 0.0f || intensity <= 0.0f) {
          n[1]++;
          continue;
        }
        const float NdotL = saturate_f(dot3v(s.N, Ll));
        if (NdotL <= 0.0f) {
          n[2]++;
          continue;
        }
        n[3]++;
        float diffuse[3], specular[3];
        brdf(s, Ll, diffuse, specular);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float radiance = (l.color[c] * attenuation) * intensity;
          total[c] += ((diffuse[c] + specular[c]) * radiance) * NdotL;
        }
      }
    }
  }
}

// step 12's store: B10G11R11, or R16G16B16A16 Sfloat with a transparent background
template <bool TRANSPARENT>
OXC_DEV void store_colour(void* out, size_t pix, const float* color, uint32_t alpha_half) {
  if (TRANSPARENT) {
    static_cast<uint2*>(out)[pix] = make_uint2(channel_half(color[0]) | (channel_half(color[1]) << 16), channel_half(color[2]) | (alpha_half << 16));
  } else {
    static_cast<uint32_t*>(out)[pix] = pack_ufloat<6>(color[0]) | (pack_ufloat<6>(color[1]) << 11) | (pack_ufloat<5>(color[2]) << 22);
  }
}

// rule F of oxc_apply_pbr_atmosphere: the face-local clamp bilinear of the cube at direction r
OXC_DEV Texel cube_sample(const uint2* cube, uint32_t cs, const V3& r) {
  const float ax = __builtin_fabsf(r.x), ay = __builtin_fabsf(r.y), az = __builtin_fabsf(r.z);
  uint32_t face;
  float sc, tc, ma;
  if (az >= ax && az >= ay) {
    const bool neg = r.z < 0.0f;
    face = neg ? 5u : 4u, sc = neg ? -r.x : r.x, tc = -r.y, ma = r.z;
  } else if (ay >= ax) {
    const bool neg = r.y < 0.0f;
    face = neg ? 3u : 2u, sc = r.x, tc = neg ? -r.z : r.z, ma = r.y;
  } else {
    const bool neg = r.x < 0.0f;
    face = neg ? 1u : 0u, sc = neg ? r.z : -r.z, tc = -r.y, ma = r.x;
  }
  const float am = __builtin_fabsf(ma);
  return sample_rgba(cube + (size_t)face * cs * cs, cs, cs, (sc / am) * 0.5f + 0.5f, (tc / am) * 0.5f + 0.5f);
}

// rule E: sample_aerial_perspective (sky.slang:258-293) at the pixel's uv for the camera-relative position `rel`; aerial.rgb * aerial.a
OXC_DEV V3 aerial_perspective(const PbrAtmosphereArgs& a, float u, float v, const V3& rel) {
  const float relative_depth = fmaxf(0.0f, len3(rel.x, rel.y, rel.z) - a.aerial_start_km);
  const float linear_slice = relative_depth * a.inv_per_slice_depth;
  const float linear_w = linear_slice * a.inv_aerial_depth;
  const float non_linear_w = __builtin_sqrtf(linear_w);
  const float non_linear_slice = non_linear_w * a.aerial_depth;
  float weight = 1.0f;
  if (non_linear_slice < 0.70710678118654752f) weight = saturate_f((non_linear_slice * non_linear_slice) * 2.0f);
  weight = weight * saturate_f(relative_depth * a.near_depth_fade_out);
  const Axis az = axis_at<false>(non_linear_w, a.aerial_depth, (int)a.ad - 1);
  const size_t slice = (size_t)a.aw * a.ah;
  const Texel t0 = sample_rgba(a.aerial + (size_t)az.i0 * slice, a.aw, a.ah, u, v), t1 = sample_rgba(a.aerial + (size_t)az.i1 * slice, a.aw, a.ah, u, v);
  V3 c = lerp3(t0.c, t1.c, az.f);
  float w = lerp_f(t0.a, t1.a, az.f);
  c = {c.x * weight, c.y * weight, c.z * weight};
  w = 1.0f - (weight * (1.0f - w));
  c = {c.x * a.aerial_exposure, c.y * a.aerial_exposure, c.z * a.aerial_exposure};
  return {c.x * w, c.y * w, c.z * w};
}

// rule D: the colour of a sky pixel.  The binary64 closed forms (acos, atan2, exp) live here only: a wave without a sky pixel skips them.
OXC_DEV void sky_pixel(const PbrAtmosphereArgs& a, const V3& V, const V3& sun_transmittance, float* color) {
  const V3 L = {a.g.sun[0], a.g.sun[1], a.g.sun[2]}, up = {0.0f, 1.0f, 0.0f}, nV = {-V.x, -V.y, -V.z};
  const V3 eye = {0.0f, a.eye_altitude, 0.0f};
  const V3 right = normalize3(crossv(up, nV));
  const V3 forward = normalize3(crossv(right, up));
  const float lx = dot3v(L, forward), ly = dot3v(L, right);
  const float len = __builtin_sqrtf(lx * lx + ly * ly);
  const bool hit = intersect_nearest(eye, nV, a.planet_radius).has;
  float u, v;
  sky_view_lut_uv(a.zenith_horizon_angle, a.beta, a.vw, a.vh, hit, dot3v(nV, up), lx / len, ly / len, u, v);
  Texel s = sample_rgba(a.sky_view, a.vw, a.vh, u, v);
  if (!hit) {  // draw_sun(-V, L, 1.0)
    const float ct = dot3v(nV, L);
    float disc = 1.0f;
    if (!(ct >= a.min_cos)) {
      const float offset = a.min_cos - ct;
      const float gaussian = exp_rule(-offset * 50000.0f) * 0.5f;
      const float inv = (1.0f / (0.02f + offset * 300.0f)) * 0.01f;
      disc = gaussian + inv;
    }
    const float li = disc * a.g.sun_intensity;
    s.c = {s.c.x + li * sun_transmittance.x, s.c.y + li * sun_transmittance.y, s.c.z + li * sun_transmittance.z};
  }
  color[0] = s.c.x * s.a, color[1] = s.c.y * s.a, color[2] = s.c.z * s.a;
}
}  // namespace

template <bool STATS, bool TRANSPARENT>
__global__ __launch_bounds__(256) void k_pbr_apply(PbrApplyArgs a) {
  __shared__ float s_srgb[256];
  __shared__ SpotTerms s_spot[kLightChunk];
  const uint32_t tid = threadIdx.x;
  s_srgb[tid] = srgb_decode(tid);
  __syncthreads();

  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  const bool inside = px < a.w && py < a.h;
  const size_t pix = inside ? (size_t)py * a.w + px : 0;
  const bool has_sun = (a.flags & OXC_SCENE_HAS_DIRECTIONAL_LIGHT) != 0u, has_contact = (a.flags & OXC_SCENE_HAS_CONTACT_SHADOWS) != 0u,
             has_sky = (a.flags & OXC_SCENE_HAS_SKY) != 0u;

  // 1. transparent empty
  const float depth = inside ? a.depth[pix] : 1.0f;
  const bool transparent_empty = TRANSPARENT && inside && depth == 0.0f;
  bool shade = inside && !transparent_empty;  // the pixel runs rules 2-12
  if (STATS && transparent_empty) atomicAdd(&a.stats[0], 1u);
  float color[3] = {0.0f, 0.0f, 0.0f};
  const uint32_t alpha_half = transparent_empty ? 0u : 0x3C00u;  // binary16 1.0, or 0.0 beside the three zero channels of the transparent empty pixel

  Pixel p = {};
  float indirect[3] = {0.0f, 0.0f, 0.0f}, total[3] = {0.0f, 0.0f, 0.0f};
  if (shade) {
    decode_and_frame(a, s_srgb, px, py, pix, depth, p);
    // 5. sky
    if (has_sky && depth == 0.0f) {
      color[0] = a.sky_color[0], color[1] = a.sky_color[1], color[2] = a.sky_color[2];
      shade = false;
      if (STATS) atomicAdd(&a.stats[1], 1u);
    }
    if (shade) {
      // 7. surface, 6. terms, 8. ambient
      float ABx, ABy, spec_occlusion;
      surface_terms(p, ABx, ABy, spec_occlusion);
      const float lambert = 1.0f / kPi;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float kS = p.s.F0[c] * ABx + ABy;
        const float kD = (1.0f - p.s.metallic) * (1.0f - kS);
        const float ibl_diffuse = ((kD * a.env[c]) * p.s.albedo[c]) * lambert;
        const float ibl_specular = (kS * a.env[c]) * spec_occlusion;
        indirect[c] = ibl_diffuse * p.occlusion + ibl_specular;
      }
    }
  }

  // 9. lights
  uint32_t n[4] = {0, 0, 0, 0};
  walk_lights(a, s_spot, tid, shade, p.s, p.world, total, n);

  if (shade) {
    // 11. sun
    float horizon = saturate_f(1.0f + 1.3f * dot3v(p.R, p.smooth));
    horizon = horizon * horizon;
    float surface[3] = {0.0f, 0.0f, 0.0f};
    if (p.NoL > 0.0f) {
      const float visibility = (has_sun ? a.resolved[pix] : 1.0f) * (has_contact ? a.contact[pix] : 1.0f);
      const float direct = has_sun ? a.sun_intensity : 0.0f;
      float diffuse[3], specular[3];
      brdf(p.s, {a.sun[0], a.sun[1], a.sun[2]}, diffuse, specular);
#pragma unroll
      for (int c = 0; c < 3; c++) surface[c] = (((diffuse[c] + specular[c] * horizon) * direct) * p.NoL) * visibility;
    }
    // 12. colour
#pragma unroll
    for (int c = 0; c < 3; c++) color[c] = ((surface[c] + total[c]) + indirect[c]) + p.emission[c];
    if (STATS) {
      atomicAdd(&a.stats[depth == 0.0f ? 2 : p.NoL > 0.0f ? 3 : 4], 1u);
      atomicAdd(&a.stats[5], n[0]);
      atomicAdd(&a.stats[6], n[1]);
      atomicAdd(&a.stats[7], n[2]);
      atomicAdd(&a.stats[8], n[3]);
    }
  }
  if (!inside) return;
  store_colour<TRANSPARENT>(a.out, pix, color, alpha_half);
}

// The atmosphere branch (include/oxcull.h, oxc_apply_pbr_atmosphere): k_pbr_apply's shape and its decode, frame,
// surface, light loop and BRDF.  After the frame every pixel takes the sun's transmittance at its own altitude (four taps of the
// transmittance LUT); a sky pixel then runs the sky arm and is done, a lit pixel takes eight taps of the aerial LUT and two times four
// of the cube straight from global memory (both stay in L2: a block's taps touch far less than a full copy would stage).
template <bool TRANSPARENT>
__global__ __launch_bounds__(256) void k_pbr_apply_atmosphere(PbrAtmosphereArgs a) {
  __shared__ float s_srgb[256];
  __shared__ SpotTerms s_spot[kLightChunk];
  const PbrApplyArgs& g = a.g;
  const uint32_t tid = threadIdx.x;
  s_srgb[tid] = srgb_decode(tid);
  __syncthreads();

  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  const bool inside = px < g.w && py < g.h;
  const size_t pix = inside ? (size_t)py * g.w + px : 0;
  const bool has_sun = (g.flags & OXC_SCENE_HAS_DIRECTIONAL_LIGHT) != 0u, has_contact = (g.flags & OXC_SCENE_HAS_CONTACT_SHADOWS) != 0u;

  // A. transparent empty
  const float depth = inside ? g.depth[pix] : 1.0f;
  const bool transparent_empty = TRANSPARENT && inside && depth == 0.0f;
  bool shade = inside && !transparent_empty;
  float color[3] = {0.0f, 0.0f, 0.0f};
  const uint32_t alpha_half = transparent_empty ? 0u : 0x3C00u;

  Pixel p = {};
  float direct[3] = {0.0f, 0.0f, 0.0f}, aerial[3] = {0.0f, 0.0f, 0.0f}, indirect[3] = {0.0f, 0.0f, 0.0f}, total[3] = {0.0f, 0.0f, 0.0f};
  if (shade) {
    decode_and_frame(g, s_srgb, px, py, pix, depth, p);
    // C. sun
    const float world_eye_y = fmaxf(p.world.y * 0.01f + a.min_altitude, a.min_altitude);
    const V3 st = transmittance_sample(a.transmittance, a.tw, a.th, a.planet_radius, a.atmos_radius, a.h_atmos, world_eye_y, a.sun_cos_theta);
    direct[0] = (st.x * g.sun_intensity) * a.horizon_darkening;
    direct[1] = (st.y * g.sun_intensity) * a.horizon_darkening;
    direct[2] = (st.z * g.sun_intensity) * a.horizon_darkening;
    if (depth == 0.0f) {
      // D. sky pixel
      sky_pixel(a, p.s.V, st, color);
      shade = false;
    } else {
      // E. aerial perspective
      const float u = ((float)px + 0.5f) / g.fw, v = ((float)py + 0.5f) / g.fh;
      const V3 ap = aerial_perspective(a, u, v, {(p.world.x - g.camera[0]) * 0.01f, (p.world.y - g.camera[1]) * 0.01f, (p.world.z - g.camera[2]) * 0.01f});
      aerial[0] = ap.x, aerial[1] = ap.y, aerial[2] = ap.z;
      // F, G. sky ambient
      const float t = 1.0f - p.roughness;
      const V3 reflection_dir = normalize3({lerp_f(p.s.N.x, p.R.x, t), lerp_f(p.s.N.y, p.R.y, t), lerp_f(p.s.N.z, p.R.z, t)});
      const Texel spec = cube_sample(a.cube, a.cube_size, reflection_dir), diff = cube_sample(a.cube, a.cube_size, p.s.N);
      const float specular_sky[3] = {(spec.c.x * spec.a) * a.horizon_darkening, (spec.c.y * spec.a) * a.horizon_darkening, (spec.c.z * spec.a) * a.horizon_darkening};
      const float diffuse_sky[3] = {(diff.c.x * diff.a) * a.horizon_darkening, (diff.c.y * diff.a) * a.horizon_darkening, (diff.c.z * diff.a) * a.horizon_darkening};
      // H. surface, ambient
      float ABx, ABy, spec_occlusion;
      surface_terms(p, ABx, ABy, spec_occlusion);
      const float lambert = 1.0f / kPi;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float kS = p.s.F0[c] * ABx + ABy;
        const float kD = (1.0f - p.s.metallic) * (1.0f - kS);
        const float ibl_diffuse = ((kD * diffuse_sky[c]) * p.s.albedo[c]) * lambert;
        const float ibl_specular = (kS * specular_sky[c]) * spec_occlusion;
        indirect[c] = ibl_diffuse * p.occlusion + ibl_specular;
      }
    }
  }

  // I. lights
  uint32_t n[4] = {0, 0, 0, 0};
  walk_lights(g, s_spot, tid, shade, p.s, p.world, total, n);

  if (shade) {
    // J. sun term
    float horizon = saturate_f(1.0f + 1.3f * dot3v(p.R, p.smooth));
    horizon = horizon * horizon;
    float surface[3] = {0.0f, 0.0f, 0.0f};
    if (p.NoL > 0.0f) {
      const float visibility = (has_sun ? g.resolved[pix] : 1.0f) * (has_contact ? g.contact[pix] : 1.0f);
      float diffuse[3], specular[3];
      brdf(p.s, {g.sun[0], g.sun[1], g.sun[2]}, diffuse, specular);
#pragma unroll
      for (int c = 0; c < 3; c++) surface[c] = (((diffuse[c] + specular[c] * horizon) * direct[c]) * p.NoL) * visibility;
    }
    // K. colour
#pragma unroll
    for (int c = 0; c < 3; c++) color[c] = (((surface[c] + total[c]) + indirect[c]) + p.emission[c]) + aerial[c];
  }
  if (!inside) return;
  store_colour<TRANSPARENT>(g.out, pix, color, alpha_half);
}

void launch_pbr_apply(const PbrApplyArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  const bool transparent = (a.flags & OXC_SCENE_TRANSPARENT_BACKGROUND) != 0u;
  if (a.stats) {
    if (transparent)
      hipLaunchKernelGGL((k_pbr_apply<true, true>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((k_pbr_apply<true, false>), grid, dim3(256), 0, s, a);
  } else {
    if (transparent)
      hipLaunchKernelGGL((k_pbr_apply<false, true>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((k_pbr_apply<false, false>), grid, dim3(256), 0, s, a);
  }
}

// What of oxc_apply_pbr_atmosphere's rule depends on the call alone, in the binary32 operations the header states (this file is compiled
// without contraction on the host side too).  Reads a.g.sun; the AtmosphereConstants come from atmosphere_constants().
void pbr_atmosphere_constants(const oxc_atmosphere& A, PbrAtmosphereArgs& a) {
  a.tw = A.transmittance_lut_size[0], a.th = A.transmittance_lut_size[1];
  a.vw = A.sky_view_lut_size[0], a.vh = A.sky_view_lut_size[1];
  a.aw = A.aerial_perspective_lut_size[0], a.ah = A.aerial_perspective_lut_size[1], a.ad = A.aerial_perspective_lut_size[2];
  a.planet_radius = A.planet_radius, a.atmos_radius = A.atmos_radius;
  a.min_altitude = A.planet_radius + 0.001f;
  a.sun_cos_theta = (a.g.sun[0] * 0.0f + a.g.sun[1] * 1.0f) + a.g.sun[2] * 0.0f;
  const float s = fminf(fmaxf((a.sun_cos_theta - -0.1f) / (0.3f - -0.1f), 0.0f), 1.0f);
  a.horizon_darkening = (s * s) * (3.0f - 2.0f * s);
  a.min_cos = cos_rule((1.0f * kPi) / 180.0f);
  const float lut_x = (float)a.aw, lut_z = (float)a.ad;
  const float per_slice_depth = lut_x / lut_z;
  a.aerial_depth = lut_z;
  a.inv_per_slice_depth = 1.0f / per_slice_depth;
  a.inv_aerial_depth = 1.0f / lut_z;
  a.near_depth_fade_out = 1.0f / 0.001f;
  a.aerial_start_km = A.aerial_perspective_start_km;
  a.aerial_exposure = A.aerial_perspective_exposure;
}

void launch_pbr_apply_atmosphere(const PbrAtmosphereArgs& a, hipStream_t s) {
  const dim3 grid((a.g.w + 15u) / 16u, (a.g.h + 15u) / 16u);
  if (a.g.flags & OXC_SCENE_TRANSPARENT_BACKGROUND)
    hipLaunchKernelGGL((k_pbr_apply_atmosphere<true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((k_pbr_apply_atmosphere<false>), grid, dim3(256), 0, s, a);
}

}  // namespace oxc
