// oxcull_debug_view.hip -- the debug views of the visbuffer, the G-buffer and the VSM page table (gfx950): RendererInstance::apply_debug_view
// (Oxylus/src/Render/Passes/Debug.cpp:9-153, passes/debug_view.slang and passes/rmvsm_debug.slang) as one compute launch.  Rules:
// include/oxcull.h, oxc_apply_debug_view (steps V1 - V4 and R1 - R5); design and measurements: DESIGN.md section 27.
//
//   k_debug_view<VIEW>   one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block), the view a template argument chosen on
//                        the host, so a view's kernel holds its own colour rule and loads only what that rule reads.  The outline (V4)
//                        wants log2(depth + 1) * 10 -- a binary64 evaluation -- of the nine texels around a pixel: the block computes each
//                        texel's density once into an 18 x 18 LDS tile (the 16 x 16 pixels and a one-texel apron), a NaN standing for a tap
//                        that adds nothing (outside the image, or a ~0u texel; the rule itself never gives a NaN), and every pixel reads
//                        its nine from there.  Rows are 24 floats apart: a 32-bit LDS read is served in two groups of 32 lanes over 32 banks,
//                        a group is four rows of the 8 x 8 wave tile, and row * 24 mod 32 = 0 24 16 8 puts them on banks 0-7, 24-31, 16-23
//                        and 8-15, no two alike (a stride of 18 gives 0 18 4 22: rows 0 and 2 share banks 4-7, rows 1 and 3 banks 22-25).
//                        The Albedo view keeps the 256 results of the sRGB decode in LDS, as k_pbr_apply does.
//   k_debug_view_vsm     the RMVSM view: the shape of k_vsm_resolve_shadow's first half -- the clipmap records in LDS, the per-call constants
//                        in the kernel arguments -- and at most one page-table word per pixel.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction.  The wave's FP16 denormal
// mode stays at its default (the ambient-occlusion and normal halves may be denormal).
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {
namespace {
constexpr float kTau = 6.283185307179586f;
constexpr uint32_t kHalfOne = 0x3C00u;
constexpr int kTileSide = 18, kTileStride = 24;
constexpr uint32_t kVisible = 1u, kDirty = 2u, kBacked = 4u;

// debug_view.slang:31-39
OXC_DEV uint32_t hash_u32(uint32_t a) {
  a = (a + 0x7ed55d16u) + (a << 12);
  a = (a ^ 0xc761c23cu) ^ (a >> 19);
  a = (a + 0x165667b1u) + (a << 5);
  a = (a + 0xd3a2646cu) ^ (a << 9);
  a = (a + 0xfd7046c5u) + (a << 3);
  a = (a ^ 0xb55a4f09u) ^ (a >> 16);
  return a;
}
OXC_DEV V3 hash_colour(uint32_t a) {
  const uint32_t h = hash_u32(a);
  return {(float)(h & 255u) / 255.0f, (float)((h >> 8) & 255u) / 255.0f, (float)((h >> 16) & 255u) / 255.0f};
}

// hsv_to_rgb((hue, 1.0, 0.5)), debug_view.slang:25-29
OXC_DEV float hsv_channel(float n, float q) {
  const float k = fmodf(n + q, 6.0f);  // exact; NaN for a non-finite operand
  return 0.5f - (0.5f * 1.0f) * fmaxf(0.0f, fminf(k, fminf(4.0f - k, 1.0f)));
}
OXC_DEV V3 hsv_half(float hue) {
  const float q = hue / 1.0471975512f;
  return {hsv_channel(5.0f, q), hsv_channel(3.0f, q), hsv_channel(1.0f, q)};
}

// debug_view.slang:41-52, one channel
OXC_DEV float inferno_channel(float t, float c0, float c1, float c2, float c3, float c4, float c5, float c6) {
  return c0 + t * (c1 + t * (c2 + t * (c3 + t * (c4 + t * (c5 + t * c6)))));
}

OXC_DEV uint2 pack_halves(float r, float g, float b, uint32_t alpha_half) {
  return make_uint2(channel_half(r) | (channel_half(g) << 16), channel_half(b) | (alpha_half << 16));
}

// V2: the colour of view VIEW at pixel `pix`
template <uint32_t VIEW>
OXC_DEV V3 view_colour(const DebugViewArgs& a, const float* s_srgb, size_t pix, uint32_t texel) {
  if (VIEW == OXC_DEBUG_VIEW_TRIANGLES) return hash_colour(texel & 0xFFu);
  if (VIEW == OXC_DEBUG_VIEW_MESHLETS) return hash_colour(texel >> 8);
  if (VIEW == OXC_DEBUG_VIEW_MATERIALS || VIEW == OXC_DEBUG_VIEW_MESH_INSTANCES || VIEW == OXC_DEBUG_VIEW_MESH_LODS) {
    const uint32_t instance = texel >> 8;
    uint32_t mesh_index = 0u, lod_index = 0u, material_index = 0u, lod_count = 0u;  // V3: all-zero records beyond the count
    if (instance < a.meshlet_instance_count) {
      const GpuMeshInstance* mi = a.mesh_instances + a.meshlet_instances[instance].mesh_instance_index;
      mesh_index = mi->mesh_index;
      if (VIEW == OXC_DEBUG_VIEW_MATERIALS) material_index = mi->material_index;
      if (VIEW == OXC_DEBUG_VIEW_MESH_LODS) {
        lod_index = mi->lod_index;
        lod_count = a.meshes[mesh_index].lod_count;
      }
    }
    if (VIEW == OXC_DEBUG_VIEW_MATERIALS) return hash_colour(material_index);
    if (VIEW == OXC_DEBUG_VIEW_MESH_INSTANCES) return hash_colour(mesh_index);
    return hsv_half(((float)lod_index / (float)(lod_count + 1u)) * kTau);
  }
  if (VIEW == OXC_DEBUG_VIEW_OVERDRAW) {
    const float draw_scale = fminf(fmaxf(a.heatmap_scale, 0.0f), 100.0f) / 100.0f;
    const float heat = 1.0f - exp2_rule((-(float)a.overdraw[pix]) * draw_scale);
    const float t = saturate_f(heat);
    return {inferno_channel(t, 0.0002189403691192265f, 0.1065134194856116f, 11.60249308247187f, -41.70399613139459f, 77.162935699427f, -71.31942824499214f,
                            25.13112622477341f),
            inferno_channel(t, 0.001651004631001012f, 0.5639564367884091f, -3.972853965665698f, 17.43639888205313f, -33.40235894210092f, 32.62606426397723f,
                            -12.24266895238567f),
            inferno_channel(t, -0.01948089843709184f, 3.932712388889277f, -15.9423941062914f, 44.35414519872813f, -81.80730925738993f, 73.20951985803202f,
                            -23.07032500287172f)};
  }
  if (VIEW == OXC_DEBUG_VIEW_ALBEDO) {
    const uint32_t w = a.albedo[pix];
    return {s_srgb[w & 0xFFu], s_srgb[(w >> 8) & 0xFFu], s_srgb[(w >> 16) & 0xFFu]};
  }
  if (VIEW == OXC_DEBUG_VIEW_NORMAL || VIEW == OXC_DEBUG_VIEW_GEOMETRIC_NORMAL) {
    const uint2 w = a.normal[pix];
    const V3 n = oct_to_vec3(VIEW == OXC_DEBUG_VIEW_NORMAL ? w.x : w.y);
    return {n.x * 0.5f + 0.5f, n.y * 0.5f + 0.5f, n.z * 0.5f + 0.5f};
  }
  if (VIEW == OXC_DEBUG_VIEW_EMISSIVE) {
    const uint32_t w = a.emissive[pix];
    return {unpack_ufloat<6>(w & 0x7FFu), unpack_ufloat<6>((w >> 11) & 0x7FFu), unpack_ufloat<5>(w >> 22)};
  }
  if (VIEW == OXC_DEBUG_VIEW_GTAO) {
    const float v = dequantize_half(a.ao[pix]);
    return {v, v, v};
  }
  // Metallic, Roughness, BakedOcclusion: byte 0, 1, 2
  const float v = (float)((a.mro[pix] >> ((VIEW - OXC_DEBUG_VIEW_METALLIC) * 8u)) & 0xFFu) / 255.0f;
  return {v, v, v};
}

template <uint32_t VIEW>
__global__ __launch_bounds__(256) void k_debug_view(DebugViewArgs a) {
  __shared__ float s_density[kTileSide * kTileStride];
  __shared__ float s_srgb[VIEW == OXC_DEBUG_VIEW_ALBEDO ? 256 : 1];
  const uint32_t tid = threadIdx.x;
  if (VIEW == OXC_DEBUG_VIEW_ALBEDO) s_srgb[tid] = srgb_decode(tid);

  // V4, first half: the density of every texel of the tile and its apron, once
  const int x0 = (int)(blockIdx.x * 16u) - 1, y0 = (int)(blockIdx.y * 16u) - 1;
  for (uint32_t i = tid; i < (uint32_t)(kTileSide * kTileSide); i += 256u) {
    const uint32_t ty = i / (uint32_t)kTileSide, tx = i - ty * (uint32_t)kTileSide;
    const int x = x0 + (int)tx, y = y0 + (int)ty;
    float s = __builtin_nanf("");  // adds nothing
    if (x >= 0 && y >= 0 && x < (int)a.w && y < (int)a.h) {
      const size_t p = (size_t)y * a.w + (size_t)x;
      if (a.vis[p] != ~0u) s = (float)log2_f64(a.depth[p] + 1.0f) * 10.0f;
    }
    s_density[ty * (uint32_t)kTileStride + tx] = s;
  }
  __syncthreads();

  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const size_t pix = (size_t)py * a.w + px;
  const uint32_t texel = a.vis[pix];
  // V1
  if (texel == ~0u) {
    if (a.clear) a.out[pix] = make_uint2(0u, kHalfOne << 16);
    return;
  }
  // V2, V3
  const V3 c = view_colour<VIEW>(a, s_srgb, pix, texel);

  // V4, second half: the nine taps in the order of sample_offset
  const float* centre = s_density + (py - blockIdx.y * 16u + 1u) * (uint32_t)kTileStride + (px - blockIdx.x * 16u + 1u);
  float gx = 0.0f, gy = 0.0f;
#pragma unroll
  for (int tap = 0; tap < 9; tap++) {
    const int dx = tap % 3 - 1, dy = 1 - tap / 3;
    const float wx = (float)((1 - tap % 3) * (tap / 3 == 1 ? 2 : 1));  // 1 0 -1 2 0 -2 1 0 -1
    const float wy = (float)((1 - tap / 3) * (tap % 3 == 1 ? 2 : 1));  // 1 2 1 0 0 0 -1 -2 -1
    const float s = centre[dy * kTileStride + dx];
    if (s == s) {
      gx = gx + wx * s;
      gy = gy + wy * s;
    }
  }
  const float k = 1.0f - fmaxf(__builtin_fabsf(gx), __builtin_fabsf(gy));
  a.out[pix] = pack_halves(saturate_f(c.x * k), saturate_f(c.y * k), saturate_f(c.z * k), kHalfOne);
}

template <uint32_t VIEW>
void launch_view(const DebugViewArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_view<VIEW>, dim3((a.w + 15u) / 16u, (a.h + 15u) / 16u), dim3(256), 0, s, a);
}
}  // namespace

__global__ __launch_bounds__(256) void k_debug_view_vsm(DebugViewVsmArgs a) {
  __shared__ float cms[16 * 19];
  for (uint32_t i = threadIdx.x; i < a.layers * 19u; i += blockDim.x) cms[i] = a.clipmaps[i];
  __syncthreads();
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const size_t pix = (size_t)py * a.w + px;
  const float d = a.depth[pix];
  // R1
  if (d == 0.0f) {
    a.out[pix] = make_uint2(kHalfOne | (kHalfOne << 16), kHalfOne | (kHalfOne << 16));
    return;
  }
  // R2
  const float u = ((float)px + 0.5f) / (float)a.w, v = ((float)py + 0.5f) / (float)a.h;
  V3 world;
  const int ci = pixel_world_and_clipmap(a, u, v, d, world);
  const float* c = cms + ci * 19;
  const float hx = row1(c, 0, world.x, world.y, world.z), hy = row1(c, 1, world.x, world.y, world.z), hw = row1(c, 3, world.x, world.y, world.z);
  const float su = (hx / hw + 1.0f) * 0.5f, sv = (hy / hw + 1.0f) * 0.5f;
  // R3
  const bool inside = su >= 0.0f && su <= 1.0f && sv >= 0.0f && sv <= 1.0f;  // false for a NaN
  const uint32_t last = a.page_size - 1u;
  const uint32_t tx = inside ? (uint32_t)(int)floorf(su * a.fphys) % a.page_size : last, ty = inside ? (uint32_t)(int)floorf(sv * a.fphys) % a.page_size : last;
  // R4
  if (tx < 2u || ty < 2u || tx > a.page_size - 2u || ty > a.page_size - 2u) {
    const V3 rgb = hsv_half(((float)ci / a.hue_divisor) * kTau);
    a.out[pix] = pack_halves(rgb.x, rgb.y, rgb.z, kHalfOne);
    return;
  }
  // R5 (`inside` holds here: an outside pixel's texel is page_size - 1)
  uint32_t wx, wy, e = 0u;
  if (wrapped_page(c, su, sv, a.fn, (int)a.n, wx, wy)) e = a.page_table[((uint32_t)ci * a.n + wy) * a.n + wx];
  const bool backed = (e & kBacked) != 0u, dirty = (e & kDirty) != 0u, visible = (e & kVisible) != 0u;
  const uint32_t r = (backed || visible) ? kHalfOne : 0u, g = (backed || !visible) && dirty ? kHalfOne : 0u, b = backed && visible ? kHalfOne : 0u;
  a.out[pix] = make_uint2(r | (g << 16), b | (kHalfOne << 16));
}

void launch_debug_view(uint32_t view, const DebugViewArgs& a, hipStream_t s) {
  switch (view) {
    case OXC_DEBUG_VIEW_TRIANGLES: return launch_view<OXC_DEBUG_VIEW_TRIANGLES>(a, s);
    case OXC_DEBUG_VIEW_MESHLETS: return launch_view<OXC_DEBUG_VIEW_MESHLETS>(a, s);
    case OXC_DEBUG_VIEW_OVERDRAW: return launch_view<OXC_DEBUG_VIEW_OVERDRAW>(a, s);
    case OXC_DEBUG_VIEW_MATERIALS: return launch_view<OXC_DEBUG_VIEW_MATERIALS>(a, s);
    case OXC_DEBUG_VIEW_MESH_INSTANCES: return launch_view<OXC_DEBUG_VIEW_MESH_INSTANCES>(a, s);
    case OXC_DEBUG_VIEW_MESH_LODS: return launch_view<OXC_DEBUG_VIEW_MESH_LODS>(a, s);
    case OXC_DEBUG_VIEW_ALBEDO: return launch_view<OXC_DEBUG_VIEW_ALBEDO>(a, s);
    case OXC_DEBUG_VIEW_NORMAL: return launch_view<OXC_DEBUG_VIEW_NORMAL>(a, s);
    case OXC_DEBUG_VIEW_EMISSIVE: return launch_view<OXC_DEBUG_VIEW_EMISSIVE>(a, s);
    case OXC_DEBUG_VIEW_METALLIC: return launch_view<OXC_DEBUG_VIEW_METALLIC>(a, s);
    case OXC_DEBUG_VIEW_ROUGHNESS: return launch_view<OXC_DEBUG_VIEW_ROUGHNESS>(a, s);
    case OXC_DEBUG_VIEW_BAKED_OCCLUSION: return launch_view<OXC_DEBUG_VIEW_BAKED_OCCLUSION>(a, s);
    case OXC_DEBUG_VIEW_GTAO: return launch_view<OXC_DEBUG_VIEW_GTAO>(a, s);
    default: return launch_view<OXC_DEBUG_VIEW_GEOMETRIC_NORMAL>(a, s);  // the host has checked the range
  }
}

void launch_debug_view_vsm(const DebugViewVsmArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_view_vsm, dim3((a.w + 15u) / 16u, (a.h + 15u) / 16u), dim3(256), 0, s, a);
}

}  // namespace oxc
