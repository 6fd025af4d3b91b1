// oxcull_terrain_maps.hip -- the terrain maps (gfx950): the three compute passes of Terrain::bake (Scene/Terrain.cpp:406-461) and of the
// brush's regional re-bake (Passes/Terrain.cpp:134-156): passes/terrain_generate.slang with terrain.slang, passes/terrain_derive.slang and
// passes/terrain_minmax.slang.  Rules: include/oxcull.h, oxc_generate_terrain_maps (steps T1 - T12); design: DESIGN.md section 24.
//
//   k_terrain_generate   one texel per lane, an 8 x 8 tile per wave, 16 x 16 per block: the reference's work group.  A texel runs its noise
//                        octaves and its erosion octaves serially (every octave reads the one before), 16 cells per erosion octave, each a
//                        hash, an exp and a cos / sin pair by the closed binary64 rules.  Nothing is shared between lanes.
//   k_terrain_derive     one texel per lane, the same tiles: nine unorm16 loads with the clamp, the Sobel, four smoothsteps, two stores.
//   k_terrain_minmax     one wave per patch, four patches per block: the lanes stride over the patch's texels, then a butterfly over the wave.
//                        The reduction runs on the u16 texels: q -> f32(q) / 65535.0f is monotonic, so the min / max of the loads is the load
//                        of the min / max, and 65535 and 0 are the seed (1.0, 0.0).
//
// The origins come from device memory (a.region) in every kernel: the grid is sized from the dispatch arguments alone.
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_terrain_device.hpp"  // hash2 (T2), noised (T3), clamp_lo_hi: shared with the terrain brush

namespace oxc {

// what depends on the call alone, in the binary32 operations of the header block
void terrain_maps_constants(TerrainMapsArgs& a) {
  const oxc_terrain_erosion& E = a.g.erosion;
  for (int c = 0; c < 2; c++) {
    a.fres[c] = (float)a.res[c];
    a.den[c] = 8.0f * a.d.texel_world_size[c];
    a.mm_scale[c] = (float)a.res[c] / (float)a.patches[c];
  }
  a.strength0 = E.strength * E.scale;
  a.freq0 = 1.0f / (E.scale * E.cell_scale);
  a.one_minus_norm = 1.0f - E.normalization;
  a.amp06 = a.g.height_amplitude * 0.6f;
}

namespace {
constexpr float kTau = 6.283185307179586476925286766559f;
constexpr float kEpsilon = 1e-10f;  // TERRAIN_EPSILON

OXC_DEV float ease_out(float t) {
  const float v = 1.0f - saturate_f(t);
  return 1.0f - v * v;
}
OXC_DEV float smooth_start(float t, float s) { return t >= s ? t - 0.5f * s : ((0.5f * t) * t) / s; }
OXC_DEV float smoothstep_f(float e0, float e1, float x) {
  const float s = saturate_f((x - e0) / (e1 - e0));
  return (s * s) * (3.0f - 2.0f * s);
}

// A binary32 value as an operand of its own.  Without it the compiler fuses a product with the binary16 conversion that follows into
// v_fma_mixlo_f16 (a * b + 0), and the +0 addend turns a product of -0 into +0.
OXC_DEV float opaque(float x) {
  asm("" : "+v"(x));
  return x;
}

// the origin pair of a kernel: words `first`, `first + 1` of the region record, or zero without one
OXC_DEV uint2 origin_of(const uint32_t* region, int first) { return region ? make_uint2(region[first], region[first + 1]) : make_uint2(0u, 0u); }

// T1 - T9
__global__ __launch_bounds__(256) void k_terrain_generate(TerrainMapsArgs a) {
  const uint2 t = tile_pixel();
  const uint2 o = origin_of(a.region, 0);
  const uint32_t tx = o.x + t.x, ty = o.y + t.y;
  if (tx >= a.res[0] || ty >= a.res[1]) return;
  const oxc_terrain_generate& G = a.g;
  const oxc_terrain_erosion& E = G.erosion;
  const float px = (((float)tx + 0.5f) / a.fres[0]) * G.domain_size, py = (((float)ty + 0.5f) / a.fres[1]) * G.domain_size;

  // T4
  V3 r = {0.0f, 0.0f, 0.0f};
  float amplitude = 1.0f, nfreq = G.height_frequency;
#pragma unroll 1
  for (uint32_t i = 0; i < G.height_octaves; i++) {
    const float fs = (float)(E.seed + i);
    const V3 oct = noised(px * nfreq, py * nfreq, fs * 0.06711056f, fs * 0.00583715f);
    const float af = amplitude * nfreq;
    r.x = r.x + oct.x * amplitude;
    r.y = r.y + oct.y * af;
    r.z = r.z + oct.z * af;
    amplitude = amplitude * G.height_gain;
    nfreq = nfreq * G.height_lacunarity;
  }
  // T5
  const float bx0 = r.x * G.height_amplitude, by = r.y * G.height_amplitude, bz = r.z * G.height_amplitude;
  const float fade_target = clamp_lo_hi(bx0 / a.amp06, -1.0f, 1.0f);
  const float bx = bx0 * 0.5f + 0.5f;

  // T6
  float strength = a.strength0, freq = a.freq0;
  float target = clamp_lo_hi(fade_target, -1.0f, 1.0f);
  float height = bx;
  const float slope_length = fmaxf(__builtin_sqrtf(by * by + bz * bz), kEpsilon);
  float magnitude = 0.0f, rounding_mult = 1.0f;
  const float rounding_for_input = lerp_f(E.rounding[1], E.rounding[0], saturate_f(target + 0.5f)) * E.rounding[2];
  float combi_mask = ease_out(smooth_start(slope_length * E.onset[0], rounding_for_input * E.onset[0]));
  float ridge_mask = ease_out(slope_length * E.onset[2]);
  float ridge_target = target;
  float gx = lerp_f(by, (by / slope_length) * E.assumed_slope[0], E.assumed_slope[1]);
  float gy = lerp_f(bz, (bz / slope_length) * E.assumed_slope[0], E.assumed_slope[1]);
  const float phase_offset = 0.25f * kTau;

#pragma unroll 1
  for (uint32_t i = 0; i < E.octaves; i++) {
    // T7
    const float fs = (float)(E.seed + i);
    const float sx = fs * 0.06711056f, sy = fs * 0.00583715f;
    const float len = __builtin_sqrtf(gx * gx + gy * gy);
    const bool keep = len > kEpsilon;
    const float nx = keep ? gx / len : 0.0f, ny = keep ? gy / len : 0.0f;
    const float side_x = ((ny * -1.0f) * E.cell_scale) * kTau, side_y = ((nx * 1.0f) * E.cell_scale) * kTau;
    const float ppx = px * freq, ppy = py * freq;
    const float cx = floorf(ppx), cy = floorf(ppy);
    const float fx = ppx - cx, fy = ppy - cy;
    float dir_x = 0.0f, dir_y = 0.0f, weight_sum = 0.0f;
#pragma unroll 1
    for (int ca = -1; ca <= 2; ca++) {
#pragma unroll 1
      for (int cb = -1; cb <= 2; cb++) {
        const float ga = (float)ca, gb = (float)cb;
        const V2 h = hash2(cx + ga, cy + gb, sx, sy);
        const float dx = (fx - ga) - h.x * 0.5f, dy = (fy - gb) - h.y * 0.5f;
        const float sq = dx * dx + dy * dy;
        const float weight = fmaxf(0.0f, exp_rule((-sq) * 2.0f) - 0.01111f);
        weight_sum = weight_sum + weight;
        const float w = (dx * side_x + dy * side_y) + phase_offset;
        float cs, sn;
        cos_sin_angle_rule(w, cs, sn);
        dir_x = dir_x + cs * weight;
        dir_y = dir_y + sn * weight;
      }
    }
    const float wden = fmaxf(weight_sum, kEpsilon);
    const float ipx = dir_x / wden, ipy = dir_y / wden;
    const float pmag = fmaxf(a.one_minus_norm, __builtin_sqrtf(ipx * ipx + ipy * ipy));
    const float phx = ipx / pmag, phy = ipy / pmag;
    // T8
    const float phz = side_x * (-freq), phw = side_y * (-freq);
    const float sloping = __builtin_fabsf(phy);
    const float sg = sign_f(phy);
    gx = gx + ((sg * phz) * strength) * E.gully_weight;
    gy = gy + ((sg * phw) * strength) * E.gully_weight;
    const float faded = lerp_f(target, phx * E.gully_weight, combi_mask);
    height = height + faded * strength;
    magnitude = magnitude + strength;
    target = faded;
    const float rounding_for_octave = lerp_f(E.rounding[1], E.rounding[0], saturate_f(phx + 0.5f)) * rounding_mult;
    const float new_mask = ease_out(smooth_start(sloping * E.onset[1], rounding_for_octave * E.onset[1]));
    combi_mask = (1.0f - pow_rule(1.0f - saturate_f(combi_mask), E.detail)) * new_mask;
    ridge_target = lerp_f(ridge_target, phx, ridge_mask);
    ridge_mask = ridge_mask * ease_out(sloping * E.onset[3]);
    strength = strength * E.gain;
    freq = freq * E.lacunarity;
    rounding_mult = rounding_mult * E.rounding[3];
  }
  // T9
  const float delta = height - bx;
  const float ridge = opaque(ridge_target * (1.0f - ridge_mask));
  const float offset = lerp_f(G.height_offset[0], -fade_target, G.height_offset[1]) * magnitude;
  const float h = (bx + delta) + offset;
  const size_t at = (size_t)ty * a.res[0] + tx;
  a.heightmap[at] = (uint16_t)cvt_u32_sat(floorf(saturate_f(h + a.height_edit[at]) * 65535.0f + 0.5f));
  a.ridgemap[at] = (uint16_t)channel_half(ridge);
}

OXC_DEV float load_height(const TerrainMapsArgs& a, int x, int y) {
  const int cx = clamp_i(x, 0, (int)a.res[0] - 1), cy = clamp_i(y, 0, (int)a.res[1] - 1);
  return (float)a.heightmap[(size_t)cy * a.res[0] + cx] / 65535.0f;
}

// T10, T11
__global__ __launch_bounds__(256) void k_terrain_derive(TerrainMapsArgs a) {
  const uint2 t = tile_pixel();
  const uint2 o = origin_of(a.region, 0);
  const uint32_t tx = o.x + t.x, ty = o.y + t.y;
  if (tx >= a.res[0] || ty >= a.res[1]) return;
  const oxc_terrain_derive& D = a.d;
  const int x = (int)tx, y = (int)ty;
  const float h00 = load_height(a, x - 1, y - 1), h10 = load_height(a, x, y - 1), h20 = load_height(a, x + 1, y - 1);
  const float h01 = load_height(a, x - 1, y), h21 = load_height(a, x + 1, y);
  const float h02 = load_height(a, x - 1, y + 1), h12 = load_height(a, x, y + 1), h22 = load_height(a, x + 1, y + 1);
  const float dhdx = ((((h20 + 2.0f * h21) + h22) - ((h00 + 2.0f * h01) + h02)) * D.height_range) / a.den[0];
  const float dhdz = ((((h02 + 2.0f * h12) + h22) - ((h00 + 2.0f * h10) + h20)) * D.height_range) / a.den[1];
  const V3 normal = normalize3({-dhdx, 1.0f, -dhdz});
  const size_t at = (size_t)ty * a.res[0] + tx;
  a.normalmap[at] = channel_half(normal.x) | (channel_half(normal.z) << 16);

  const float height = load_height(a, x, y);
  const float ridge = dequantize_half(a.ridgemap[at]);
  const float slope = saturate_f(1.0f - normal.y);
  const float rock = smoothstep_f(D.slope_rock_begin, D.slope_rock_end, slope);
  const float snow = smoothstep_f(D.altitude_snow_begin, D.altitude_snow_end, height) * (1.0f - rock);
  const float drainage = (saturate_f((-ridge) * D.ridge_drainage_scale) * (1.0f - rock)) * (1.0f - snow);
  const float grass = saturate_f(((1.0f - rock) - snow) - drainage);
  const uint32_t pw = a.splat_edit[at];
  const float p0 = (float)(pw & 0xFFu) / 255.0f, p1 = (float)((pw >> 8) & 0xFFu) / 255.0f, p2 = (float)((pw >> 16) & 0xFFu) / 255.0f, p3 = (float)(pw >> 24) / 255.0f;
  const float w0 = saturate_f(((1.0f - p0) - p1) - p2);
  a.splatmap[at] = pack_unorm(lerp_f(grass, w0, p3)) | (pack_unorm(lerp_f(rock, p0, p3)) << 8) | (pack_unorm(lerp_f(drainage, p1, p3)) << 16) |
                   (pack_unorm(lerp_f(snow, p2, p3)) << 24);
}

// T12
__global__ __launch_bounds__(256) void k_terrain_minmax(TerrainMapsArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // a block holds the four patches of a 4 x 1 strip; index = the Slang's thread_id.xy
  const uint32_t ix = blockIdx.x * 4u + wave, iy = blockIdx.y;
  const uint2 o = origin_of(a.region, 2);
  const uint32_t px = o.x + ix, py = o.y + iy;
  if (px >= a.patches[0] || py >= a.patches[1]) return;  // wave-uniform
  const uint32_t bx = cvt_u32_sat(floorf((float)px * a.mm_scale[0])), by = cvt_u32_sat(floorf((float)py * a.mm_scale[1]));
  const uint32_t ex = min(cvt_u32_sat(ceilf((float)(px + 1u) * a.mm_scale[0])) + 1u, a.res[0]);
  const uint32_t ey = min(cvt_u32_sat(ceilf((float)(py + 1u) * a.mm_scale[1])) + 1u, a.res[1]);
  uint32_t lo = 65535u, hi = 0u;
  if (ex > bx && ey > by) {
    const uint32_t w = ex - bx, n = w * (ey - by);  // at most 16384^2 = 2^28
    for (uint32_t k = lane; k < n; k += 64u) {
      const uint32_t yy = k / w, xx = k - yy * w;
      const uint32_t q = a.heightmap[(size_t)(by + yy) * a.res[0] + (bx + xx)];
      lo = min(lo, q);
      hi = max(hi, q);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, m, 64));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, m, 64));
  }
  if (lane == 0u) a.patch_minmax[(size_t)py * a.patches[0] + px] = make_float2((float)lo / 65535.0f, (float)hi / 65535.0f);
}
}  // namespace

void launch_terrain_generate(const TerrainMapsArgs& a, hipStream_t s) {
  if (!a.threads_texels[0] || !a.threads_texels[1]) return;
  hipLaunchKernelGGL(k_terrain_generate, dim3(a.threads_texels[0] / 16u, a.threads_texels[1] / 16u), dim3(256), 0, s, a);
}

void launch_terrain_derive(const TerrainMapsArgs& a, hipStream_t s) {
  if (!a.threads_texels[0] || !a.threads_texels[1]) return;
  hipLaunchKernelGGL(k_terrain_derive, dim3(a.threads_texels[0] / 16u, a.threads_texels[1] / 16u), dim3(256), 0, s, a);
}

void launch_terrain_minmax(const TerrainMapsArgs& a, hipStream_t s) {
  if (!a.threads_patches[0] || !a.threads_patches[1]) return;
  hipLaunchKernelGGL(k_terrain_minmax, dim3(a.threads_patches[0] / 4u, a.threads_patches[1]), dim3(256), 0, s, a);
}

}  // namespace oxc
