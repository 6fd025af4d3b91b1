// oxcull_visbuffer_decode.hip -- the G-buffer images from the visibility buffer (gfx950): RendererInstance::decode_visbuffer
// (Oxylus/src/Render/Passes/DrawGeometry.cpp:192-274, passes/visbuffer_decode.slang) as one compute launch -- the geometry and material-factor
// half of the shader; texture sampling and everything that only feeds it are out of scope.  Rules: include/oxcull.h, oxc_decode_visbuffer;
// design and measurements: DESIGN.md section 15.
//
//   k_visbuffer_decode   one thread per pixel, an 8 x 8 pixel tile per wave (a 16 x 16 tile per block), as the other per-pixel passes: the
//                        pixels of a tile mostly show the same few triangles, so the five dependent loads of the fetch chain (meshlet
//                        instance -> mesh instance -> mesh -> LOD -> meshlet -> micro indices -> vertex ids -> vertices) hit lines the
//                        first lane brought in.  An empty pixel is two loads and, with `clear`, four stores.  No LDS, no scratch.
//                        Steps 1 - 5, the factor unpack and the packing of the words are oxcull_decode_device.hpp's, the one copy
//                        k_visbuffer_decode_textured runs too; what is left here is the order of the stages.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and square
// root are the IEEE ones, pow is the ambient occlusion's closed form in binary64.  The wave's FP16 denormal mode stays at its default
// (denormals kept: the normal image holds denormal halves), so the flush of com::dequantize_half is spelled out (dequantize_half_flush);
// the kernel must not call set_half_denorm_flush().
#include <hip/hip_runtime.h>

#include "oxcull_decode_device.hpp"

namespace oxc {

namespace {
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

  // 1. empty pixel, 2. fetch chain
  DecodedPixel<false> p;
  const int outcome = decode_fetch(a, pix, p);
  if (outcome != kDecoded) {
    count<STATS>(a, outcome);
    return;
  }

  // the material's five words (all zero beyond material_count), ahead of the world matrix
  uint32_t mw[5] = {0u, 0u, 0u, 0u, 0u};
  if (p.material_index < a.material_count) {
    const uint32_t* rec = a.materials + (size_t)p.material_index * 14u;
#pragma unroll
    for (int k = 0; k < 5; k++) mw[k] = rec[k];
  } else {
    count<STATS>(a, kDefaultMaterial);
  }

  // 3. positions and normals, 4. clip positions and barycentrics, 5. normal
  decode_interpolate(a, nullptr, px, py, p);
  const uint32_t oct = oct_halves(p.wnrm);
  a.normal[pix] = make_uint2(oct, oct);

  // 6. albedo, 7. metallic / roughness / occlusion, 8. emissive
  const MaterialFactors f = material_factors(mw);
  a.albedo[pix] = pack_albedo(f.ar, f.ag, f.ab, f.aa);
  a.emissive[pix] = pack_emissive(f.er, f.eg, f.eb);
  a.mro[pix] = pack_mro(f.metallic, f.roughness, 1.0f);
  count<STATS>(a, kDecoded);
}

void launch_visbuffer_decode(const VisbufferDecodeArgs& a, hipStream_t s) {
  const dim3 grid((a.w + 15u) / 16u, (a.h + 15u) / 16u);
  if (a.stats)
    hipLaunchKernelGGL(k_visbuffer_decode<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_visbuffer_decode<false>, grid, dim3(256), 0, s, a);
}

}  // namespace oxc
