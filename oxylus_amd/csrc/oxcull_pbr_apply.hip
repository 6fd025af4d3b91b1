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

OXC_DEV float dot3v(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
OXC_DEV float clamp_f(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// the cos rule of oxc_apply_pbr: binary64, two-constant reduction, the polynomials of cos_sin_turn, one rounding
OXC_DEV float cos_rule(float x) {
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

// one channel of the sRGB decode
OXC_DEV float srgb_decode(uint32_t byte) {
  const float c = (float)byte / 255.0f;
  return c <= 0.04045f ? c / 12.92f : pow_rule((c + 0.055f) / 1.055f, 2.4f);
}

// com::oct_to_vec3 of the two halves of `word` (the first in the low half): one normalisation
OXC_DEV V3 oct_to_vec3(uint32_t word) { return normalize3(oct_normal_ba(word)); }

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
  const GpuLight* __restrict__ lights = static_cast<const GpuLight*>(a.lights);
  const bool has_sun = (a.flags & OXC_SCENE_HAS_DIRECTIONAL_LIGHT) != 0u, has_contact = (a.flags & OXC_SCENE_HAS_CONTACT_SHADOWS) != 0u,
             has_sky = (a.flags & OXC_SCENE_HAS_SKY) != 0u;

  // 1. transparent empty
  const float depth = inside ? a.depth[pix] : 1.0f;
  const bool transparent_empty = TRANSPARENT && inside && depth == 0.0f;
  bool shade = inside && !transparent_empty;  // the pixel runs rules 2-12
  if (STATS && transparent_empty) atomicAdd(&a.stats[0], 1u);
  float color[3] = {0.0f, 0.0f, 0.0f};
  const uint32_t alpha_half = transparent_empty ? 0u : 0x3C00u;  // binary16 1.0, or 0.0 beside the three zero channels of the transparent empty pixel

  Surface s = {};
  V3 world = {0.0f, 0.0f, 0.0f}, smooth = {0.0f, 0.0f, 0.0f}, R = {0.0f, 0.0f, 0.0f};
  float emission[3] = {0.0f, 0.0f, 0.0f}, indirect[3] = {0.0f, 0.0f, 0.0f}, total[3] = {0.0f, 0.0f, 0.0f};
  float NoL = 0.0f;
  if (shade) {
    // 2. decode
    const uint32_t albedo_w = a.albedo[pix];
    const uint2 normal_w = a.normal[pix];
    const uint32_t emissive_w = a.emissive[pix], mro_w = a.mro[pix];
    const uint32_t ao_h = a.ao[pix];
    s.albedo[0] = s_srgb[albedo_w & 0xFFu], s.albedo[1] = s_srgb[(albedo_w >> 8) & 0xFFu], s.albedo[2] = s_srgb[(albedo_w >> 16) & 0xFFu];
    const V3 mapped = oct_to_vec3(normal_w.x);
    smooth = oct_to_vec3(normal_w.y);
    emission[0] = unpack_ufloat<6>(emissive_w & 0x7FFu), emission[1] = unpack_ufloat<6>((emissive_w >> 11) & 0x7FFu), emission[2] = unpack_ufloat<5>(emissive_w >> 22);
    s.metallic = clamp_f((float)(mro_w & 0xFFu) / 255.0f, 0.0f, 1.0f);
    const float roughness = clamp_f((float)((mro_w >> 8) & 0xFFu) / 255.0f, 0.045f, 1.0f);
    const float occlusion = ((float)((mro_w >> 16) & 0xFFu) / 255.0f) * dequantize_half(ao_h);
    // 3. position
    const float u = ((float)px + 0.5f) / a.fw, v = ((float)py + 0.5f) / a.fh;
    unproject(a.inv_pv, u, v, depth, world.x, world.y, world.z);
    // 4. frame
    s.V = normalize3({a.camera[0] - world.x, a.camera[1] - world.y, a.camera[2] - world.z});
    s.N = normalize3(mapped);
    const V3 nV = {-s.V.x, -s.V.y, -s.V.z};
    const float two_d = 2.0f * dot3v(s.N, nV);
    R = {nV.x - two_d * s.N.x, nV.y - two_d * s.N.y, nV.z - two_d * s.N.z};
    s.NoV = __builtin_fabsf(dot3v(s.N, s.V)) + 1e-5f;
    NoL = fmaxf(dot3v(s.N, {a.sun[0], a.sun[1], a.sun[2]}), 0.0f);
    // 5. sky
    if (has_sky && depth == 0.0f) {
      color[0] = a.sky_color[0], color[1] = a.sky_color[1], color[2] = a.sky_color[2];
      shade = false;
      if (STATS) atomicAdd(&a.stats[1], 1u);
    }
    if (shade) {
      // 7. surface
      const float alpha = fmaxf(roughness * roughness, 0.0025f);
      s.alpha2 = alpha * alpha;
      const float x = s.NoV, y = alpha, x2 = x * x, y2 = y * y;
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; k++)
        r[k] = (((((((kAlbedoFit[0][k] + kAlbedoFit[1][k] * x) + kAlbedoFit[2][k] * y) + (kAlbedoFit[3][k] * x) * y) + kAlbedoFit[4][k] * x2) + kAlbedoFit[5][k] * y2) +
                 (kAlbedoFit[6][k] * x2) * y) +
                (kAlbedoFit[7][k] * x) * y2) +
               (kAlbedoFit[8][k] * x2) * y2;
      const float ABx = clamp_f(r[0] / r[2], 0.0f, 1.0f), ABy = clamp_f(r[1] / r[3], 0.0f, 1.0f);
      const float Ess = saturate_f(ABx + ABy);
      // 6. terms, 8. ambient
      const float spec_occlusion = saturate_f((pow_rule(s.NoV + occlusion, exp2_rule(-16.0f * roughness - 1.0f)) - 1.0f) + occlusion);
      const float lambert = 1.0f / kPi;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        s.F0[c] = 0.04f + (s.albedo[c] - 0.04f) * s.metallic;
        s.ec[c] = 1.0f + (s.F0[c] * (1.0f - Ess)) / fmaxf(Ess, 1e-4f);
        const float kS = s.F0[c] * ABx + ABy;
        const float kD = (1.0f - s.metallic) * (1.0f - kS);
        const float ibl_diffuse = ((kD * a.env[c]) * s.albedo[c]) * lambert;
        const float ibl_specular = (kS * a.env[c]) * spec_occlusion;
        indirect[c] = ibl_diffuse * occlusion + ibl_specular;
      }
    }
  }

  // 9. lights, in chunks: a barrier, one light's pixel-independent terms per thread, a barrier, then every shading pixel walks the chunk
  uint32_t n_kind = 0, n_att = 0, n_ndl = 0, n_shaded = 0;
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
          n_kind++;
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
          n_att++;
          continue;
        }
        const float NdotL = saturate_f(dot3v(s.N, Ll));
        if (NdotL <= 0.0f) {
          n_ndl++;
          continue;
        }
        n_shaded++;
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

  if (shade) {
    // 11. sun
    float horizon = saturate_f(1.0f + 1.3f * dot3v(R, smooth));
    horizon = horizon * horizon;
    float surface[3] = {0.0f, 0.0f, 0.0f};
    if (NoL > 0.0f) {
      const float visibility = (has_sun ? a.resolved[pix] : 1.0f) * (has_contact ? a.contact[pix] : 1.0f);
      const float direct = has_sun ? a.sun_intensity : 0.0f;
      float diffuse[3], specular[3];
      brdf(s, {a.sun[0], a.sun[1], a.sun[2]}, diffuse, specular);
#pragma unroll
      for (int c = 0; c < 3; c++) surface[c] = (((diffuse[c] + specular[c] * horizon) * direct) * NoL) * visibility;
    }
    // 12. colour
#pragma unroll
    for (int c = 0; c < 3; c++) color[c] = ((surface[c] + total[c]) + indirect[c]) + emission[c];
    if (STATS) {
      atomicAdd(&a.stats[depth == 0.0f ? 2 : NoL > 0.0f ? 3 : 4], 1u);
      atomicAdd(&a.stats[5], n_kind);
      atomicAdd(&a.stats[6], n_att);
      atomicAdd(&a.stats[7], n_ndl);
      atomicAdd(&a.stats[8], n_shaded);
    }
  }
  if (!inside) return;
  if (TRANSPARENT) {
    static_cast<uint2*>(a.out)[pix] = make_uint2(channel_half(color[0]) | (channel_half(color[1]) << 16), channel_half(color[2]) | (alpha_half << 16));
  } else {
    static_cast<uint32_t*>(a.out)[pix] = pack_ufloat<6>(color[0]) | (pack_ufloat<6>(color[1]) << 11) | (pack_ufloat<5>(color[2]) << 22);
  }
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

}  // namespace oxc
