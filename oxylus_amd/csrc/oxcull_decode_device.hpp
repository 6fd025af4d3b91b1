// oxcull_decode_device.hpp -- the device rules the decodes of the visibility buffer share, one copy each: steps 1 - 5 of oxc_decode_visbuffer
// (include/oxcull.h) for k_visbuffer_decode (oxcull_visbuffer_decode.hip) and k_visbuffer_decode_textured (oxcull_visbuffer_decode_textured.hip),
// the unpacking of a material's factor words for the two, and the packing of the G-buffer words for them and k_terrain_decode
// (oxcull_terrain_decode.hip).  Every float operation keeps the order and rounding the header states; the including files are compiled
// without contraction.  The wave's FP16 denormal mode stays at its default (denormals kept: the normal image holds denormal halves), so the
// flush of com::dequantize_half is dequantize_half_flush; no includer may call set_half_denorm_flush().
#pragma once

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

// What became of a pixel in steps 1 - 2, and with kDefaultMaterial the counters stats[0 .. 3] of both decodes
// (oxc_debug_visbuffer_decode_stats; the textured decode's further counters continue at kDecodeCounters)
enum : int { kDecoded = 0, kEmpty, kZeroVertexIndex, kDefaultMaterial, kDecodeCounters };

// Mesh::decode_normal, scene.slang:486-489
OXC_DEV V3 decode_mesh_normal(uint32_t packed) {
  return {(float)((packed >> 20) & 1023u) / 511.0f - 1.0f, (float)((packed >> 10) & 1023u) / 511.0f - 1.0f, (float)(packed & 1023u) / 511.0f - 1.0f};
}

// The four images of a cleared or rejected pixel
OXC_DEV void store_zero_pixel(const VisbufferDecodeArgs& a, size_t pix) {
  a.albedo[pix] = 0u;
  a.normal[pix] = make_uint2(0u, 0u);
  a.emissive[pix] = 0u;
  a.mro[pix] = 0u;
}

// One pixel through steps 1 - 5: decode_fetch fills the first group, decode_interpolate the rest.  TEXTURED adds what only the sampling
// of steps 9 - 14 reads; without it none of those loads or values exists.
template <bool TEXTURED>
struct DecodedPixel {
  uint64_t positions, normals;  // the mesh's streams
  uint32_t vi[3];               // the triangle's vertex indices, all within the mesh
  uint32_t material_index, transform_index;
  V3 wnrm;                      // world_normal
};
// Step 4's results that step 10 reads: the lambdas, the interpolated 1 / w and the barycentric derivatives before their rescaling
struct Barycentrics {
  float l[3], interp_inv_w, ddx[3], ddy[3], ddx_sum, ddy_sum;
};
template <>
struct DecodedPixel<true> : DecodedPixel<false> {
  uint64_t texcoords;  // the mesh's stream
  V3 crw[3];           // camera-relative world positions
  float tu[3], tv[3];  // step 9: the vertices' texcoords
  Barycentrics bary;
};

// Steps 1 - 2 of pixel `pix`: kEmpty (cleared when the call clears), kZeroVertexIndex (zeros stored) or kDecoded.  The caller counts.
template <bool TEXTURED>
OXC_DEV int decode_fetch(const VisbufferDecodeArgs& a, size_t pix, DecodedPixel<TEXTURED>& p) {
  const uint32_t texel = a.vis[pix];
  const uint32_t depth_bits = a.depth_bits[pix];
  const uint32_t instance = texel >> 8, triangle = texel & 0xFFu;

  // 1. empty pixel
  if (texel == ~0u || instance == kTerrainInstanceId || depth_bits == 0u || instance >= a.meshlet_instance_count) {
    if (a.clear) store_zero_pixel(a, pix);
    return kEmpty;
  }

  // 2. fetch chain (visbuffer_decode.slang:95-103) and Meshlet::indices
  const GpuMeshletInstance mli = a.meshlet_instances[instance];
  const GpuMeshInstance* mi = a.mesh_instances + mli.mesh_instance_index;
  const uint32_t mesh_index = mi->mesh_index, lod_index = mi->lod_index;
  p.material_index = mi->material_index, p.transform_index = mi->transform_index;
  const GpuMesh* mesh = a.meshes + mesh_index;
  p.positions = mesh->vertex_positions, p.normals = mesh->vertex_normals;
  if constexpr (TEXTURED) p.texcoords = mesh->texture_coords;
  const uint64_t lods = mesh->lods;
  const uint32_t vertex_count = mesh->vertex_count;
  const uint64_t lod = lods + (uint64_t)lod_index * sizeof(GpuMeshLOD);
  const uint2 meshlets2 = load_global_u2(lod, 1), micro2 = load_global_u2(lod, 3), vidx2 = load_global_u2(lod, 4);  // GpuMeshLOD's pointers
  const uint64_t meshlets = meshlets2.x | ((uint64_t)meshlets2.y << 32), micro = micro2.x | ((uint64_t)micro2.y << 32),
                 vidx = vidx2.x | ((uint64_t)vidx2.y << 32);
  const uint4 meshlet = load_global_u4(meshlets, mli.meshlet_index);  // {vertex offset, triangle offset, vertex count, triangle count}
  const uint32_t base = meshlet.y + triangle * 3u;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint32_t byte = base + k;
    const uint32_t local = (load_global_u32(micro, byte >> 2) >> ((byte & 3u) * 8u)) & 0xFFu;
    p.vi[k] = load_global_u32(vidx, meshlet.x + local);
  }
  const uint32_t last = vertex_count - 1u;  // wraps for vertex_count == 0, as in the Slang
  if (p.vi[0] > last || p.vi[1] > last || p.vi[2] > last) {
    store_zero_pixel(a, pix);
    return kZeroVertexIndex;
  }
  return kDecoded;
}

// Steps 3 - 5 of a pixel decode_fetch decoded, and with TEXTURED step 9's loads.  `camera_position` is read with TEXTURED alone.
template <bool TEXTURED>
OXC_DEV void decode_interpolate(const VisbufferDecodeArgs& a, const float* camera_position, uint32_t px, uint32_t py, DecodedPixel<TEXTURED>& p) {
  float world[16];
  {
    const float4* t = reinterpret_cast<const float4*>(a.transforms) + (size_t)p.transform_index * 4u;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const float4 col = t[c];
      world[c * 4 + 0] = col.x, world[c * 4 + 1] = col.y, world[c * 4 + 2] = col.z, world[c * 4 + 3] = col.w;
    }
  }

  // 3. positions and normals, 4. the three clip positions; 9. the texcoords (a null stream decodes (0, 0))
  float nm[9];
  normal_matrix(world, nm);
  float cx[3], cy[3], inv_w[3];
  V3 wn[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint2 q = load_global_u2(p.positions, p.vi[k]);
    const float lx = dequantize_half_flush(q.x & 0xFFFFu), ly = dequantize_half_flush(q.x >> 16), lz = dequantize_half_flush(q.y & 0xFFFFu);
    const float wx = row1(world, 0, lx, ly, lz), wy = row1(world, 1, lx, ly, lz), wz = row1(world, 2, lx, ly, lz);
    cx[k] = row1(a.pv, 0, wx, wy, wz);
    cy[k] = row1(a.pv, 1, wx, wy, wz);
    inv_w[k] = 1.0f / row1(a.pv, 3, wx, wy, wz);
    const V3 n = p.normals ? decode_mesh_normal(load_global_u32(p.normals, p.vi[k])) : V3{0.0f, 0.0f, 0.0f};
    wn[k] = {(nm[0] * n.x + nm[3] * n.y) + nm[6] * n.z, (nm[1] * n.x + nm[4] * n.y) + nm[7] * n.z, (nm[2] * n.x + nm[5] * n.y) + nm[8] * n.z};
    if constexpr (TEXTURED) {
      p.crw[k] = {wx - camera_position[0], wy - camera_position[1], wz - camera_position[2]};
      const uint32_t tc = p.texcoords ? load_global_u32(p.texcoords, p.vi[k]) : 0u;
      p.tu[k] = dequantize_half_flush(tc & 0xFFFFu), p.tv[k] = dequantize_half_flush(tc >> 16);
    }
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
  p.wnrm = normalize3({(l0 * wn[0].x + l1 * wn[1].x) + l2 * wn[2].x, (l0 * wn[0].y + l1 * wn[1].y) + l2 * wn[2].y,
                       (l0 * wn[0].z + l1 * wn[1].z) + l2 * wn[2].z});

  if constexpr (TEXTURED) p.bary = {{l0, l1, l2}, interp_inv_w, {ddx0, ddx1, ddx2}, {ddy0, ddy1, ddy2}, ddx_sum, ddy_sum};
}

// The factors of GPU::Material's words 0 - 4, nine halves through dequantize_half_flush
struct MaterialFactors {
  float ar, ag, ab, aa;  // albedo_color
  float er, eg, eb;      // emissive_color
  float roughness, metallic;
};
OXC_DEV MaterialFactors material_factors(const uint32_t* mw) {
  return {dequantize_half_flush(mw[0] & 0xFFFFu), dequantize_half_flush(mw[0] >> 16), dequantize_half_flush(mw[1] & 0xFFFFu), dequantize_half_flush(mw[1] >> 16),
          dequantize_half_flush(mw[2] & 0xFFFFu), dequantize_half_flush(mw[2] >> 16), dequantize_half_flush(mw[3] & 0xFFFFu),
          dequantize_half_flush(mw[3] >> 16), dequantize_half_flush(mw[4] & 0xFFFFu)};
}

// The G-buffer words: albedo R8G8B8A8 sRGB with a unorm alpha, emissive B10G11R11 UfloatPack32, metallic / roughness / occlusion R8G8B8A8 Unorm
OXC_DEV uint32_t pack_albedo(float r, float g, float b, float a) { return srgb_unorm(r) | (srgb_unorm(g) << 8) | (srgb_unorm(b) << 16) | (pack_unorm(a) << 24); }
OXC_DEV uint32_t pack_emissive(float r, float g, float b) { return pack_ufloat<6>(r) | (pack_ufloat<6>(g) << 11) | (pack_ufloat<5>(b) << 22); }
OXC_DEV uint32_t pack_mro(float metallic, float roughness, float occlusion) { return pack_unorm(metallic) | (pack_unorm(roughness) << 8) | (pack_unorm(occlusion) << 16); }

}  // namespace oxc
