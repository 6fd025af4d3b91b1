// oxcull_visbuffer_decode.hip -- the G-buffer images from the visibility buffer (gfx950): RendererInstance::decode_visbuffer
// (Oxylus/src/Render/Passes/DrawGeometry.cpp:192-274, passes/visbuffer_decode.slang) as one compute launch -- the geometry and material-factor
// half of the shader; texture sampling and everything that only feeds it are out of scope.  Rules: include/oxcull.h, oxc_decode_visbuffer;
// design and measurements: DESIGN.md section 15.
//
//   k_visbuffer_decode   one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block), as the other per-pixel passes: the
//                        pixels of a tile mostly show the same few triangles, so the five dependent loads of the fetch chain (meshlet
//                        instance -> mesh instance -> mesh -> LOD -> meshlet -> micro indices -> vertex ids -> vertices) hit lines the
//                        first lane brought in.  An empty pixel is two loads and, with `clear`, four stores.  No LDS, no scratch.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and square
// root are the IEEE ones, pow is the ambient occlusion's closed form in binary64.  The wave's FP16 denormal mode stays at its default
// (denormals kept: the normal image holds denormal halves), so the flush of com::dequantize_half is spelled out here; the kernel must not
// call set_half_denorm_flush().
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
// Mesh::decode_normal, scene.slang:486-489
OXC_DEV V3 decode_normal(uint32_t packed) {
  return {(float)((packed >> 20) & 1023u) / 511.0f - 1.0f, (float)((packed >> 10) & 1023u) / 511.0f - 1.0f, (float)(packed & 1023u) / 511.0f - 1.0f};
}

template <bool STATS>
OXC_DEV void count(const VisbufferDecodeArgs& a, int k) {
  if (STATS) atomicAdd(&a.stats[k], 1u);
}
}  // namespace

template <bool STATS>
__global__ __launch_bounds__(256) void k_visbuffer_decode(VisbufferDecodeArgs a) {
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= a.w || py >= a.h) return;
  const size_t pix = (size_t)py * a.w + px;
  const uint32_t texel = a.vis[pix];
  const uint32_t depth_bits = a.depth_bits[pix];
  const uint32_t instance = texel >> 8, triangle = texel & 0xFFu;

  // 1. empty pixel
  if (texel == ~0u || instance == kTerrainInstanceId || depth_bits == 0u || instance >= a.meshlet_instance_count) {
    if (a.clear) {
      a.albedo[pix] = 0u;
      a.normal[pix] = make_uint2(0u, 0u);
      a.emissive[pix] = 0u;
      a.mro[pix] = 0u;
    }
    count<STATS>(a, 1);
    return;
  }

  // 2. fetch chain (visbuffer_decode.slang:95-103) and Meshlet::indices
  const GpuMeshletInstance mli = a.meshlet_instances[instance];
  const GpuMeshInstance* mi = a.mesh_instances + mli.mesh_instance_index;
  const uint32_t mesh_index = mi->mesh_index, lod_index = mi->lod_index, material_index = mi->material_index, transform_index = mi->transform_index;
  const GpuMesh* mesh = a.meshes + mesh_index;
  const uint64_t positions = mesh->vertex_positions, normals = mesh->vertex_normals, lods = mesh->lods;
  const uint32_t vertex_count = mesh->vertex_count;
  const uint64_t lod = lods + (uint64_t)lod_index * sizeof(GpuMeshLOD);
  const uint2 meshlets2 = load_global_u2(lod, 1), micro2 = load_global_u2(lod, 3), vidx2 = load_global_u2(lod, 4);  // GpuMeshLOD's pointers
  const uint64_t meshlets = meshlets2.x | ((uint64_t)meshlets2.y << 32), micro = micro2.x | ((uint64_t)micro2.y << 32),
                 vidx = vidx2.x | ((uint64_t)vidx2.y << 32);
  const uint4 meshlet = load_global_u4(meshlets, mli.meshlet_index);  // {vertex offset, triangle offset, vertex count, triangle count}
  const uint32_t base = meshlet.y + triangle * 3u;
  uint32_t vi[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint32_t byte = base + k;
    const uint32_t local = (load_global_u32(micro, byte >> 2) >> ((byte & 3u) * 8u)) & 0xFFu;
    vi[k] = load_global_u32(vidx, meshlet.x + local);
  }
  const uint32_t last = vertex_count - 1u;  // wraps for vertex_count == 0, as in the Slang
  if (vi[0] > last || vi[1] > last || vi[2] > last) {
    a.albedo[pix] = 0u;
    a.normal[pix] = make_uint2(0u, 0u);
    a.emissive[pix] = 0u;
    a.mro[pix] = 0u;
    count<STATS>(a, 2);
    return;
  }

  // the material's five words (all zero beyond material_count) and the world matrix
  uint32_t mw[5] = {0u, 0u, 0u, 0u, 0u};
  if (material_index < a.material_count) {
    const uint32_t* rec = a.materials + (size_t)material_index * 14u;
#pragma unroll
    for (int k = 0; k < 5; k++) mw[k] = rec[k];
  } else {
    count<STATS>(a, 3);
  }
  float world[16];
  {
    const float4* t = reinterpret_cast<const float4*>(a.transforms) + (size_t)transform_index * 4u;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const float4 col = t[c];
      world[c * 4 + 0] = col.x, world[c * 4 + 1] = col.y, world[c * 4 + 2] = col.z, world[c * 4 + 3] = col.w;
    }
  }

  // 3. positions and normals, 4. the three clip positions
  float nm[9];
  normal_matrix(world, nm);
  float cx[3], cy[3], inv_w[3];
  V3 wn[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint2 q = load_global_u2(positions, vi[k]);
    const float lx = dequantize_half_flush(q.x & 0xFFFFu), ly = dequantize_half_flush(q.x >> 16), lz = dequantize_half_flush(q.y & 0xFFFFu);
    const float wx = row1(world, 0, lx, ly, lz), wy = row1(world, 1, lx, ly, lz), wz = row1(world, 2, lx, ly, lz);
    cx[k] = row1(a.pv, 0, wx, wy, wz);
    cy[k] = row1(a.pv, 1, wx, wy, wz);
    inv_w[k] = 1.0f / row1(a.pv, 3, wx, wy, wz);
    const V3 n = normals ? decode_normal(load_global_u32(normals, vi[k])) : V3{0.0f, 0.0f, 0.0f};
    wn[k] = {(nm[0] * n.x + nm[3] * n.y) + nm[6] * n.z, (nm[1] * n.x + nm[4] * n.y) + nm[7] * n.z, (nm[2] * n.x + nm[5] * n.y) + nm[8] * n.z};
  }

  // 4. barycentrics (visbuffer_decode.slang:45-73)
  const float n0x = cx[0] * inv_w[0], n0y = cy[0] * inv_w[0];
  const float n1x = cx[1] * inv_w[1], n1y = cy[1] * inv_w[1];
  const float n2x = cx[2] * inv_w[2], n2y = cy[2] * inv_w[2];
  const float inv_det = 1.0f / ((n2x - n1x) * (n0y - n1y) - (n2y - n1y) * (n0x - n1x));
  const float ddx0 = ((n1y - n2y) * inv_det) * inv_w[0], ddx1 = ((n2y - n0y) * inv_det) * inv_w[1], ddx2 = ((n0y - n1y) * inv_det) * inv_w[2];
  const float ddy0 = ((n2x - n1x) * inv_det) * inv_w[0], ddy1 = ((n0x - n2x) * inv_det) * inv_w[1], ddy2 = ((n1x - n0x) * inv_det) * inv_w[2];
  const float ddx_sum = (ddx0 + ddx1) + ddx2, ddy_sum = (ddy0 + ddy1) + ddy2;
  const float u = (((float)px + 0.5f) / a.fw) * 2.0f - 1.0f, v = (((float)py + 0.5f) / a.fh) * 2.0f - 1.0f;
  const float dvx = u - n0x, dvy = v - n0y;
  const float interp_inv_w = (inv_w[0] + dvx * ddx_sum) + dvy * ddy_sum;
  const float interp_w = 1.0f / interp_inv_w;
  const float l0 = interp_w * ((inv_w[0] + dvx * ddx0) + dvy * ddy0);
  const float l1 = interp_w * (dvx * ddx1 + dvy * ddy1);
  const float l2 = interp_w * (dvx * ddx2 + dvy * ddy2);

  // 5. normal
  const V3 wnrm = normalize3({(l0 * wn[0].x + l1 * wn[1].x) + l2 * wn[2].x, (l0 * wn[0].y + l1 * wn[1].y) + l2 * wn[2].y,
                              (l0 * wn[0].z + l1 * wn[1].z) + l2 * wn[2].z});
  const uint32_t oct = oct_halves(wnrm);
  a.normal[pix] = make_uint2(oct, oct);

  // 6. albedo, 7. metallic / roughness / occlusion, 8. emissive
  const float ar = dequantize_half_flush(mw[0] & 0xFFFFu), ag = dequantize_half_flush(mw[0] >> 16), ab = dequantize_half_flush(mw[1] & 0xFFFFu),
              aa = dequantize_half_flush(mw[1] >> 16);
  a.albedo[pix] = srgb_unorm(ar) | (srgb_unorm(ag) << 8) | (srgb_unorm(ab) << 16) | (pack_unorm(aa) << 24);
  const float er = dequantize_half_flush(mw[2] & 0xFFFFu), eg = dequantize_half_flush(mw[2] >> 16), eb = dequantize_half_flush(mw[3] & 0xFFFFu);
  a.emissive[pix] = pack_ufloat<6>(er) | (pack_ufloat<6>(eg) << 11) | (pack_ufloat<5>(eb) << 22);
  const float roughness = dequantize_half_flush(mw[3] >> 16), metallic = dequantize_half_flush(mw[4] & 0xFFFFu);
  a.mro[pix] = pack_unorm(metallic) | (pack_unorm(roughness) << 8) | (pack_unorm(1.0f) << 16);
  count<STATS>(a, 0);
}

void launch_visbuffer_decode(const VisbufferDecodeArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  if (a.stats)
    hipLaunchKernelGGL(k_visbuffer_decode<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_visbuffer_decode<false>, grid, dim3(256), 0, s, a);
}

}  // namespace oxc
