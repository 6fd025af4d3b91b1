// oxcull_visbuffer_decode_textured.hip -- the G-buffer images from the visibility buffer with the five material images sampled (gfx950):
// the whole of passes/visbuffer_decode.slang as one compute launch.  Rules: include/oxcull.h, oxc_decode_visbuffer_textured (steps 1 - 8 are
// oxc_decode_visbuffer's, steps 9 - 14 the texcoords, the gradients, the tangent frame, SampleGrad and the outputs); design and
// measurements: DESIGN.md section 31.
//
//   k_visbuffer_decode_textured   the shape of k_visbuffer_decode: one thread per pixel, an 8 x 8 pixel tile per wave, a 16 x 16 tile per
//                        block.  Steps 1 - 5 are oxcull_decode_device.hpp's, the one copy both kernels run, with what the sampling
//                        reads switched on (DecodedPixel<true>).  Then:
//                        - the block fills two 256-entry LDS tables, byte / 255.0f and srgb_decode(byte), one entry per thread, when the call
//                          has an image table at all: a texel channel is one LDS read, not a division or three binary64 pow;
//                        - a wave whose live lanes all name one material reads that material, its sampler and its image records through a
//                          uniform index (ballot + readfirstlane, then loads through the constant address space: scalar loads, the records in SGPRs;
//                          record_word below); every other wave reads them per lane.
//                          Both run the same shade() body and produce the same bytes;
//                        - the eight texel loads of one image (2 levels x 4 texels, all at wrapped or clamped coordinates, so every address
//                          is inside its level) are issued as one batch before the first is decoded.  A nearest filter is the linear one with
//                          both coordinates equal and weight 0, a nearest mip filter the trilinear one with both levels equal and weight 0:
//                          a + (a - a) * 0 is a for the finite values a texel decodes to.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division and square
// root are the IEEE ones, log2 and pow are the closed forms in binary64.  The wave's FP16 denormal mode stays at its default, as in
// k_visbuffer_decode.
#include <hip/hip_runtime.h>

#include "oxcull_decode_device.hpp"

namespace oxc {

namespace {
// the counters of oxc_debug_visbuffer_decode_textured_stats after the four both decodes keep
enum : int { kSampled = kDecodeCounters /* + image kind, 5 */, kLevelTaps = 9, kJacobianZero, kUniformWaves, kPerLaneWaves };
enum : uint32_t { kHasAlbedo = 1u, kHasNormal = 2u, kHasEmissive = 4u, kHasMetallicRoughness = 8u, kHasOcclusion = 16u, kNormalTwoComponent = 32u, kNormalFlipY = 64u };

template <bool STATS>
OXC_DEV void count(const VisbufferDecodeTexturedArgs& a, int k, uint32_t n = 1u) {
  if (STATS) atomicAdd(&a.g.stats[k], n);
}

struct F4 {
  float r, g, b, a;
};
struct F2 {
  float x, y;
};

// One pixel after steps 1 - 5 and 9 (the shared part: crw, wnrm and what step 10 reads) and step 10
struct Pixel : DecodedPixel<true> {
  F2 uv, ddx, ddy;      // tex_coord_grad before the material's uv_size / uv_offset
  float bx[3], by[3];   // the final ddx / ddy of compute_partial_derivatives
};

// One axis of a level tap (step 12): linear filter -> the repeat axis of oxc_apply_tonemap or axis_at<false>; nearest -> the texel at
// floor(u * size) by the same integer rule, twice, weight 0.
struct TapAxis {
  int i0, i1;
  float f;
};
OXC_DEV TapAxis tap_axis(float coord, int size, bool linear, bool clamp) {
  TapAxis t;
  if (linear) {
    if (clamp) {
      const Axis a = axis_at<false>(coord, (float)size, size - 1);
      t.i0 = a.i0, t.i1 = a.i1, t.f = a.f;
    } else {
      const WrapAxis a = wrap_axis(coord, size);
      t.i0 = a.i0, t.i1 = a.i1, t.f = a.f;
    }
  } else {
    const int i = cvt_i32_sat(floorf(coord * (float)size));
    t.i0 = t.i1 = clamp ? clamp_i(i, 0, size - 1) : floor_mod_i(i, size);
    t.f = 0.0f;
  }
  return t;
}

// One texel of a level: `w` is the row length in texels, FORMAT 2 has two bytes a texel
OXC_DEV uint32_t load_texel(uint64_t level, uint32_t format, uint32_t index) {
  if (format == 2u) return reinterpret_cast<const unsigned short __attribute__((address_space(1)))*>(level)[index];
  return load_global_u32(level, index);
}
// decode first, then filter: R8G8B8A8 Unorm byte / 255.0f; sRGB: r, g, b through srgb_decode, alpha byte / 255.0f; R8G8: b = 0, a = 1
OXC_DEV F4 decode_texel(const float* tab, uint32_t format, uint32_t word) {
  const float* rgb = tab + (format == 1u ? 256 : 0);
  F4 t;
  t.r = rgb[word & 0xFFu];
  t.g = rgb[(word >> 8) & 0xFFu];
  t.b = format == 2u ? 0.0f : rgb[(word >> 16) & 0xFFu];
  t.a = format == 2u ? 1.0f : tab[word >> 24];
  return t;
}
OXC_DEV F4 lerp4(const F4& a, const F4& b, float t) { return {lerp_f(a.r, b.r, t), lerp_f(a.g, b.g, t), lerp_f(a.b, b.b, t), lerp_f(a.a, b.a, t)}; }

// Word k of a device record.  UNIFORM: `rec` is the same in every live lane (its index went through readfirstlane), and the load goes
// through the constant address space, which the compiler turns into a scalar load: the word arrives in an SGPR.
template <bool UNIFORM>
OXC_DEV uint32_t record_word(const uint32_t* rec, int k) {
  if (UNIFORM) return reinterpret_cast<const uint32_t __attribute__((address_space(4)))*>(reinterpret_cast<uint64_t>(rec))[k];
  return rec[k];
}

// The fields of an oxc_material_image record the sampling reads first; the level offsets are read at the two levels' indices
struct ImageHead {
  uint64_t dptr;
  uint32_t width, height, levels, format;
};
// UNIFORM: `index` is the same in every live lane and the record goes through scalar registers
template <bool UNIFORM>
OXC_DEV ImageHead image_head(const VisbufferDecodeTexturedArgs& a, uint32_t index) {
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.images + (UNIFORM ? (uint32_t)__builtin_amdgcn_readfirstlane((int)index) : index));
  ImageHead h;
  const uint32_t lo = record_word<UNIFORM>(rec, 0), hi = record_word<UNIFORM>(rec, 1);
  h.dptr = lo | ((uint64_t)hi << 32);
  h.width = record_word<UNIFORM>(rec, 2), h.height = record_word<UNIFORM>(rec, 3), h.levels = record_word<UNIFORM>(rec, 4), h.format = record_word<UNIFORM>(rec, 5);
  return h;
}
// step 13's "image absent": nothing of the image is read
OXC_DEV bool image_present(const ImageHead& h) {
  return h.dptr != 0u && h.levels != 0u && h.format <= 2u && h.width - 1u < 16384u && h.height - 1u < 16384u;
}

// step 12: SampleGrad of image `index` (present: the caller asked) at uv with the gradients gx, gy under sampler (filter, address, mip_filter)
template <bool UNIFORM, bool STATS>
OXC_DEV F4 sample_grad(const VisbufferDecodeTexturedArgs& a, const float* tab, uint32_t index, const ImageHead& h, uint32_t filter, uint32_t address,
                       uint32_t mip_filter, const F2& uv, const F2& gx, const F2& gy) {
  const uint32_t levels = min(h.levels, 15u);
  const float fw0 = (float)h.width, fh0 = (float)h.height;
  const float mxx = gx.x * fw0, mxy = gx.y * fh0, myx = gy.x * fw0, myy = gy.y * fh0;
  const float rho = fmaxf(__builtin_sqrtf(mxx * mxx + mxy * mxy), __builtin_sqrtf(myx * myx + myy * myy));
  float lambda = (float)log2_f64(rho);
  lambda = lambda == lambda ? lambda : 0.0f;
  const float last = (float)(levels - 1u);
  lambda = fminf(fmaxf(lambda, 0.0f), last);
  int lo, hi;
  float t;
  if (mip_filter) {
    const float fl = floorf(lambda);
    lo = (int)fl;
    hi = min(lo + 1, (int)levels - 1);
    t = lambda - fl;
  } else {
    lo = hi = min((int)floorf(lambda + 0.5f), (int)levels - 1);
    t = 0.0f;
  }
  count<STATS>(a, kLevelTaps, mip_filter ? 2u : 1u);
  const bool linear = filter != 0u, clamp = address != 0u;
  const uint64_t rec = reinterpret_cast<uint64_t>(a.images + index);
  // both levels' addresses, then the eight loads as one batch
  uint32_t word[8];
  float fx[2], fy[2];
  uint64_t level[2];
  uint32_t at[8];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int lvl = k ? hi : lo;
    const uint2 off = load_global_u2(rec, 3u + (uint32_t)lvl);  // level_offset[lvl]
    level[k] = h.dptr + (off.x | ((uint64_t)off.y << 32));
    const int w = (int)max(1u, h.width >> lvl), hgt = (int)max(1u, h.height >> lvl);
    const TapAxis ax = tap_axis(uv.x, w, linear, clamp), ay = tap_axis(uv.y, hgt, linear, clamp);
    fx[k] = ax.f, fy[k] = ay.f;
    const uint32_t r0 = (uint32_t)ay.i0 * (uint32_t)w, r1 = (uint32_t)ay.i1 * (uint32_t)w;
    at[k * 4 + 0] = r0 + (uint32_t)ax.i0, at[k * 4 + 1] = r0 + (uint32_t)ax.i1, at[k * 4 + 2] = r1 + (uint32_t)ax.i0, at[k * 4 + 3] = r1 + (uint32_t)ax.i1;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) word[k] = load_texel(level[k >> 2], h.format, at[k]);
  F4 tap[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const F4 t00 = decode_texel(tab, h.format, word[k * 4 + 0]), t10 = decode_texel(tab, h.format, word[k * 4 + 1]);
    const F4 t01 = decode_texel(tab, h.format, word[k * 4 + 2]), t11 = decode_texel(tab, h.format, word[k * 4 + 3]);
    tap[k] = lerp4(lerp4(t00, t10, fx[k]), lerp4(t01, t11, fx[k]), fy[k]);
  }
  return lerp4(tap[0], tap[1], t);
}

// Steps 11 - 14 of one pixel under material `material_index` (UNIFORM: the same in every live lane)
template <bool UNIFORM, bool STATS>
OXC_DEV void shade(const VisbufferDecodeTexturedArgs& a, const float* tab, size_t pix, uint32_t material_index, const Pixel& p) {
  uint32_t mw[14];
#pragma unroll
  for (int k = 0; k < 14; k++) mw[k] = 0u;
  if (material_index < a.g.material_count) {
    const uint32_t* rec = a.g.materials + (size_t)(UNIFORM ? (uint32_t)__builtin_amdgcn_readfirstlane((int)material_index) : material_index) * 14u;
#pragma unroll
    for (int k = 0; k < 14; k++) mw[k] = record_word<UNIFORM>(rec, k);
  } else {
    count<STATS>(a, kDefaultMaterial);
  }
  const uint32_t flags = mw[5];
  // the material's one sampler; out of range: linear / repeat / linear-mip
  uint32_t filter = 1u, address = 0u, mip_filter = 1u;
  if (mw[6] < a.sampler_count) {
    const uint32_t* s = a.samplers + (size_t)mw[6] * 4u;
    filter = record_word<UNIFORM>(s, 0), address = record_word<UNIFORM>(s, 1), mip_filter = record_word<UNIFORM>(s, 2);
  }
  // step 10, the material's half: uv * uv_size + uv_offset, the gradients times uv_size
  const float usx = dequantize_half_flush(mw[12] & 0xFFFFu), usy = dequantize_half_flush(mw[12] >> 16);
  const float uox = dequantize_half_flush(mw[13] & 0xFFFFu), uoy = dequantize_half_flush(mw[13] >> 16);
  const F2 uv = {p.uv.x * usx + uox, p.uv.y * usy + uoy};
  const F2 gx = {p.ddx.x * usx, p.ddx.y * usy}, gy = {p.ddy.x * usx, p.ddy.y * usy};

  // step 12 for each image kind whose flag is set and whose record is present
  F4 texel[5];
  bool has[5];
#pragma unroll
  for (int kind = 0; kind < 5; kind++) {
    has[kind] = false;
    texel[kind] = {1.0f, 1.0f, 1.0f, 1.0f};
    const uint32_t index = mw[7 + kind];
    if ((flags >> kind) & 1u) {
      if (index < a.image_count) {
        const ImageHead h = image_head<UNIFORM>(a, index);
        if (image_present(h)) {
          has[kind] = true;
          count<STATS>(a, kSampled + kind);
          texel[kind] = sample_grad<UNIFORM, STATS>(a, tab, index, h, filter, address, mip_filter, uv, gx, gy);
        }
      }
    }
  }

  // step 14: albedo
  const MaterialFactors f = material_factors(mw);
  F4 albedo = {f.ar, f.ag, f.ab, f.aa};
  if (has[0]) albedo = {f.ar * texel[0].r, f.ag * texel[0].g, f.ab * texel[0].b, f.aa * texel[0].a};
  a.g.albedo[pix] = pack_albedo(albedo.r, albedo.g, albedo.b, albedo.a);

  // step 11 and the normal: the tangent frame is computed where a normal image is sampled
  const uint32_t geometric = oct_halves(p.wnrm);
  uint32_t shading = geometric;
  if (has[1]) {
    const V3& n = p.wnrm;
    V3 pos_ddx, pos_ddy;
    pos_ddx.x = (p.bx[0] * p.crw[0].x + p.bx[1] * p.crw[1].x) + p.bx[2] * p.crw[2].x;
    pos_ddx.y = (p.bx[0] * p.crw[0].y + p.bx[1] * p.crw[1].y) + p.bx[2] * p.crw[2].y;
    pos_ddx.z = (p.bx[0] * p.crw[0].z + p.bx[1] * p.crw[1].z) + p.bx[2] * p.crw[2].z;
    pos_ddy.x = (p.by[0] * p.crw[0].x + p.by[1] * p.crw[1].x) + p.by[2] * p.crw[2].x;
    pos_ddy.y = (p.by[0] * p.crw[0].y + p.by[1] * p.crw[1].y) + p.by[2] * p.crw[2].y;
    pos_ddy.z = (p.by[0] * p.crw[0].z + p.by[1] * p.crw[1].z) + p.by[2] * p.crw[2].z;
    const float dx = dot3v(pos_ddx, n), dy = dot3v(pos_ddy, n);
    const V3 sx = {pos_ddx.x - dx * n.x, pos_ddx.y - dx * n.y, pos_ddx.z - dx * n.z};
    const V3 sy = {pos_ddy.x - dy * n.x, pos_ddy.y - dy * n.y, pos_ddy.z - dy * n.z};
    const float js = sign_f(gx.x * gy.y - gx.y * gy.x);
    V3 tangent = {js * (gy.y * sx.x - gx.y * sy.x), js * (gy.y * sx.y - gx.y * sy.y), js * (gy.y * sx.z - gx.y * sy.z)};
    if (js != 0.0f)
      tangent = normalize3(tangent);
    else
      count<STATS>(a, kJacobianZero);
    const float w = js * sign_f(dot3v(pos_ddy, crossv(n, pos_ddx)));
    const V3 c = crossv(n, tangent);
    const float mw_ = -w;
    const V3 bitangent = {mw_ * c.x, mw_ * c.y, mw_ * c.z};
    float nx = texel[1].r * 2.0f - 1.0f, ny = texel[1].g * 2.0f - 1.0f, nz = texel[1].b * 2.0f - 1.0f;
    ny = (flags & kNormalFlipY) ? -ny : ny;
    nz = (flags & kNormalTwoComponent) ? __builtin_sqrtf(saturate_f(1.0f - (nx * nx + ny * ny))) : nz;
    const V3 v = {(nx * tangent.x + ny * bitangent.x) + nz * n.x, (nx * tangent.y + ny * bitangent.y) + nz * n.y, (nx * tangent.z + ny * bitangent.z) + nz * n.z};
    shading = oct_halves(normalize3(v));
  }
  a.g.normal[pix] = make_uint2(shading, geometric);

  // emissive, metallic / roughness, occlusion
  float er = f.er, eg = f.eg, eb = f.eb;
  if (has[2]) er = er * texel[2].r, eg = eg * texel[2].g, eb = eb * texel[2].b;
  a.g.emissive[pix] = pack_emissive(er, eg, eb);
  float roughness = f.roughness, metallic = f.metallic;
  if (has[3]) metallic = metallic * texel[3].b, roughness = roughness * texel[3].g;
  const float occlusion = has[4] ? texel[4].r : 1.0f;
  a.g.mro[pix] = pack_mro(metallic, roughness, occlusion);
  count<STATS>(a, kDecoded);
}
}  // namespace

template <bool STATS>
__global__ __launch_bounds__(256) void k_visbuffer_decode_textured(VisbufferDecodeTexturedArgs a) {
  // the two decode tables: [0, 256) byte / 255.0f, [256, 512) srgb_decode(byte).  A call without an image table samples nothing.
  __shared__ float tab[512];
  if (a.image_count) {
    tab[threadIdx.x] = (float)threadIdx.x / 255.0f;
    tab[256u + threadIdx.x] = srgb_decode(threadIdx.x);
    __syncthreads();
  }
  const VisbufferDecodeArgs& g = a.g;
  const uint2 tp = tile_pixel();
  const uint32_t px = tp.x, py = tp.y;
  if (px >= g.w || py >= g.h) return;
  const size_t pix = (size_t)py * g.w + px;

  // 1. empty pixel, 2. fetch chain
  Pixel p;
  const int outcome = decode_fetch(g, pix, p);
  if (outcome != kDecoded) {
    count<STATS>(a, outcome);
    return;
  }
  // 3. positions and normals, 4. clip positions and barycentrics, 5. normal; 9. the texcoords
  decode_interpolate(g, a.camera_position, px, py, p);

  // 10. the gradients (visbuffer_decode.slang:74-83) and gradient_of (:32-39)
  {
    const Barycentrics& b = p.bary;
    const float l0 = b.l[0], l1 = b.l[1], l2 = b.l[2], *tu = p.tu, *tv = p.tv;
    const float sx = 2.0f / g.fw, sy = -(2.0f / g.fh);
    const float rx0 = b.ddx[0] * sx, rx1 = b.ddx[1] * sx, rx2 = b.ddx[2] * sx, ry0 = b.ddy[0] * sy, ry1 = b.ddy[1] * sy, ry2 = b.ddy[2] * sy;
    const float rx_sum = b.ddx_sum * sx, ry_sum = b.ddy_sum * sy;
    const float interp_ddx_w = 1.0f / (b.interp_inv_w + rx_sum), interp_ddy_w = 1.0f / (b.interp_inv_w + ry_sum);
    p.bx[0] = interp_ddx_w * (l0 * b.interp_inv_w + rx0) - l0, p.bx[1] = interp_ddx_w * (l1 * b.interp_inv_w + rx1) - l1, p.bx[2] = interp_ddx_w * (l2 * b.interp_inv_w + rx2) - l2;
    p.by[0] = interp_ddy_w * (l0 * b.interp_inv_w + ry0) - l0, p.by[1] = interp_ddy_w * (l1 * b.interp_inv_w + ry1) - l1, p.by[2] = interp_ddy_w * (l2 * b.interp_inv_w + ry2) - l2;
    p.uv = {(l0 * tu[0] + l1 * tu[1]) + l2 * tu[2], (l0 * tv[0] + l1 * tv[1]) + l2 * tv[2]};
    p.ddx = {(p.bx[0] * tu[0] + p.bx[1] * tu[1]) + p.bx[2] * tu[2], (p.bx[0] * tv[0] + p.bx[1] * tv[1]) + p.bx[2] * tv[2]};
    p.ddy = {(p.by[0] * tu[0] + p.by[1] * tu[1]) + p.by[2] * tu[2], (p.by[0] * tv[0] + p.by[1] * tv[1]) + p.by[2] * tv[2]};
  }

  // the wave's live lanes all name one material: the uniform path
  const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.material_index);
  const bool uniform = __ballot(p.material_index != first) == 0ull;
  if (STATS && lane_id() == __builtin_ctzll(__ballot(1))) count<STATS>(a, uniform ? kUniformWaves : kPerLaneWaves);  // the first live lane
  if (uniform)
    shade<true, STATS>(a, tab, pix, first, p);
  else
    shade<false, STATS>(a, tab, pix, p.material_index, p);
}

void launch_visbuffer_decode_textured(const VisbufferDecodeTexturedArgs& a, hipStream_t s) {
  const dim3 grid((a.g.w + 15u) / 16u, (a.g.h + 15u) / 16u);
  if (a.g.stats)
    hipLaunchKernelGGL(k_visbuffer_decode_textured<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_visbuffer_decode_textured<false>, grid, dim3(256), 0, s, a);
}

}  // namespace oxc
