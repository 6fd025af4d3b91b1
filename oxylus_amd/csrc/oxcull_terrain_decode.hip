// oxcull_terrain_decode.hip -- the G-buffer images of the terrain pixels (gfx950): RendererInstance::decode_terrain
// (Oxylus/src/Render/Passes/Terrain.cpp:279-360, passes/terrain_decode.slang) as one compute launch -- the geometry and material-factor half
// of the shader, the cut oxc_decode_visbuffer makes; texture sampling and everything that only feeds it are out of scope.  Rules:
// include/oxcull.h, oxc_decode_terrain (steps D1 - D8); design and measurements: DESIGN.md section 26.
//
//   k_terrain_decode   one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block), as the other per-pixel passes.  A pixel
//                      that is not terrain costs its visbuffer load and leaves.  The four layer materials and the hit record are the same
//                      for every pixel of the call: their addresses are formed from kernel arguments alone, so a wave reads each once (the
//                      compiler selects scalar loads for them) and the per-layer branches on the record's kind are uniform.  The two maps
//                      are read through the clamp bilinear of the brush (map_taps): eight dependent-free loads a pixel that neighbouring
//                      lanes share.  No LDS, no scratch.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction.  The wave's FP16
// denormal mode stays at its default (the normal map and the normal image hold denormal halves), so the material factors go through
// dequantize_half_flush; the kernel must not call set_half_denorm_flush().
#include <hip/hip_runtime.h>

#include "oxcull_decode_device.hpp"
#include "oxcull_terrain_device.hpp"

namespace oxc {
namespace {
constexpr uint32_t kInvalidLayerMaterial = 0xFFFFFFFFu;  // TERRAIN_INVALID_LAYER_MATERIAL, scene.slang:632

// D5: what one splat layer adds at weight 1: albedo rgba, emissive rgb, metallic, roughness (occlusion is 1 for every kind)
struct Layer {
  float f[9];
  bool invalid;  // TERRAIN_INVALID_LAYER_MATERIAL: white, (0, 1), nothing added to emissive
};

OXC_DEV Layer layer_of(const TerrainDecodeArgs& a, int i) {
  const uint32_t index = a.t.layer_material_indices[i];
  Layer l;
  l.invalid = index == kInvalidLayerMaterial;
  uint32_t mw[5] = {0u, 0u, 0u, 0u, 0u};  // beyond material_count: the all-zero Material
  if (!l.invalid && index < a.material_count) {
    const uint32_t* rec = a.materials + (size_t)index * 14u;
#pragma unroll
    for (int k = 0; k < 5; k++) mw[k] = rec[k];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) l.f[k] = dequantize_half_flush((mw[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu);
  if (l.invalid) {
    l.f[0] = l.f[1] = l.f[2] = l.f[3] = 1.0f;
    l.f[8] = 0.0f, l.f[7] = 1.0f;  // halves 7 and 8 are roughness and metallic
  }
  return l;
}
}  // namespace

__global__ __launch_bounds__(256) void k_terrain_decode(TerrainDecodeArgs a) {
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const size_t pix = (size_t)py * a.w + px;
  // D1
  if ((a.vis[pix] >> 8) != kTerrainInstanceId) return;

  // D2
  const float u = ((float)px + 0.5f) / a.fw, v = ((float)py + 0.5f) / a.fh;
  float wx, wy, wz;
  unproject(a.ipv, u, v, a.depth[pix], wx, wy, wz);

  // D3
  const float tu = (wx - a.t.world_min[0]) * a.t.inv_world_size[0], tv = (wz - a.t.world_min[1]) * a.t.inv_world_size[1];
  const MapTaps t = map_taps(tu, tv, a.map_w, a.map_h);
  const size_t i00 = t.r0 + t.ax.i0, i10 = t.r0 + t.ax.i1, i01 = t.r1 + t.ax.i0, i11 = t.r1 + t.ax.i1;
  const float fx = t.ax.f, fy = t.ay.f;
  const uint32_t n00 = a.normalmap[i00], n10 = a.normalmap[i10], n01 = a.normalmap[i01], n11 = a.normalmap[i11];
  const uint32_t s00 = a.splatmap[i00], s10 = a.splatmap[i10], s01 = a.splatmap[i01], s11 = a.splatmap[i11];
  const float nx = lerp_f(lerp_f(dequantize_half(n00 & 0xFFFFu), dequantize_half(n10 & 0xFFFFu), fx),
                          lerp_f(dequantize_half(n01 & 0xFFFFu), dequantize_half(n11 & 0xFFFFu), fx), fy);
  const float nz = lerp_f(lerp_f(dequantize_half(n00 >> 16), dequantize_half(n10 >> 16), fx), lerp_f(dequantize_half(n01 >> 16), dequantize_half(n11 >> 16), fx), fy);
  const V3 geometric = normalize3({nx, __builtin_sqrtf(saturate_f(1.0f - (nx * nx + nz * nz))), nz});

  // D4
  float w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t sh = (uint32_t)k * 8u;
    w[k] = lerp_f(lerp_f((float)((s00 >> sh) & 0xFFu) / 255.0f, (float)((s10 >> sh) & 0xFFu) / 255.0f, fx),
                  lerp_f((float)((s01 >> sh) & 0xFFu) / 255.0f, (float)((s11 >> sh) & 0xFFu) / 255.0f, fx), fy);
  }
  const float weight_sum = ((w[0] + w[1]) + w[2]) + w[3];
  const bool weighted = weight_sum > 1e-4f;
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = weighted ? w[k] / weight_sum : (k == 0 ? 1.0f : 0.0f);

  // D5
  float albedo[4] = {0.0f, 0.0f, 0.0f, 0.0f}, emissive[3] = {0.0f, 0.0f, 0.0f}, metallic = 0.0f, roughness = 0.0f, occlusion = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const Layer l = layer_of(a, i);  // ahead of the divergent weight test on purpose: uniform addresses, so the wave reads the record once
    const float weight = w[i];
    if (weight <= 0.0f) continue;
#pragma unroll
    for (int k = 0; k < 4; k++) albedo[k] = albedo[k] + l.f[k] * weight;
    if (!l.invalid) {
#pragma unroll
      for (int k = 0; k < 3; k++) emissive[k] = emissive[k] + l.f[4 + k] * weight;
    }
    metallic = metallic + l.f[8] * weight;
    roughness = roughness + l.f[7] * weight;
    occlusion = occlusion + weight;
  }

  // D7
  if (a.t.brush_radius > 0.0f) {
    const uint2 hit_xy = reinterpret_cast<const uint2*>(a.hit)[0], hit_zw = reinterpret_cast<const uint2*>(a.hit)[1];  // one address for the whole wave
    if (hit_zw.y != 0u) {
      const float dx = wx - asf(hit_xy.x), dz = wz - asf(hit_zw.x);
      const float ring_distance = __builtin_sqrtf(dx * dx + dz * dz);
      const float ring_width = fmaxf(a.t.brush_radius * 0.02f, 0.05f);
      const float s = saturate_f((__builtin_fabsf(ring_distance - a.t.brush_radius) - 0.0f) / (ring_width - 0.0f));
      const float ring = 1.0f - (s * s) * (3.0f - 2.0f * s);
      albedo[0] = lerp_f(albedo[0], 1.0f, ring);
      albedo[1] = lerp_f(albedo[1], 0.55f, ring);
      albedo[2] = lerp_f(albedo[2], 0.1f, ring);
    }
  }

  // D6, D8
  const V3 shading = normalize3(geometric);
  a.normal[pix] = make_uint2(oct_halves(shading), oct_halves(geometric));
  a.albedo[pix] = pack_albedo(albedo[0], albedo[1], albedo[2], albedo[3]);
  a.emissive[pix] = pack_emissive(emissive[0], emissive[1], emissive[2]);
  a.mro[pix] = pack_mro(metallic, roughness, occlusion);
}

void launch_terrain_decode(const TerrainDecodeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_terrain_decode, dim3((a.w + 15u) / 16u, (a.h + 15u) / 16u), dim3(256), 0, s, a);
}

}  // namespace oxc
