// oxcull_abi_post.cpp -- the post-process and sky passes of liboxcull.so's C ABI: eye adaptation, bloom, tonemap, FXAA, the sky LUTs.
#include "oxcull_host.hpp"

namespace {
// ---- the rules of the lit HDR image the post-process passes read (final_attachment, in source_format), in the style of pixel_images.
// Every pass applies them in its own order, so each rule is a call of its own.
oxc_status post_format(oxc_ctx* ctx, const char* entry, uint32_t source_format, uint32_t& texel) {
  if (source_format > 1u) return bad_arg(ctx, entry, "source_format must be 0 (B10G11R11) or 1 (R16G16B16A16 Sfloat)");
  texel = source_format ? 8u : 4u;
  return OXC_OK;
}

// the extent rules, then the format rule
oxc_status post_source(oxc_ctx* ctx, const char* entry, uint32_t width, uint32_t height, uint32_t source_format, uint64_t& pixels, uint32_t& texel) {
  if (width == 0u || height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (width > 65536u || height > 65536u) return bad_arg(ctx, entry, "extent beyond 65536");
  pixels = (uint64_t)width * height;
  if (pixels > 0xFFFFFFFFull) return bad_arg(ctx, entry, "width * height beyond 2^32 - 1");
  return post_format(ctx, entry, source_format, texel);
}

// `b` (the field `name`) holds one texel of the source format per pixel
oxc_status post_attachment(oxc_ctx* ctx, const char* entry, const oxc_buffer& b, uint64_t pixels, uint32_t texel, const char* name = "final_attachment") {
  if (bad_pixel_buffer(b, pixels, texel)) return bad_arg(ctx, entry, name, " must be one aligned u32 per pixel (format 0) or one 8-byte aligned u16x4 per pixel (format 1)");
  return OXC_OK;
}
}  // namespace

extern "C" {

namespace {
// The pyramid contract of oxc_apply_bloom: the extent and level count, every level aligned to its texel and inside the allocation, no
// two levels sharing a byte.  `level` receives the byte span of every level.
oxc_status bloom_pyramid(oxc_ctx* ctx, const char* entry, const oxc_image_pyramid& p, const char* name, uint32_t w2, uint32_t h2, uint32_t levels, uint32_t texel,
                         ByteSpan* level) {
  if (p.width != w2 || p.height != h2 || p.levels != levels) return bad_arg(ctx, entry, name, " must have width / 2, height / 2 and floor(log2(max of them)) + 1 levels");
  const uintptr_t base = reinterpret_cast<uintptr_t>(p.dptr);
  for (uint32_t k = 0; k < levels; k++) {
    const uint64_t size = (uint64_t)std::max(1u, w2 >> k) * std::max(1u, h2 >> k) * texel, off = p.level_offset[k];
    if (!p.dptr || ((base + off) & (texel - 1u)) || off > p.bytes || size > p.bytes - off) return bad_arg(ctx, entry, name, ": every level must be aligned to its texel and lie inside the allocation");
    level[k] = {base + (uintptr_t)off, base + (uintptr_t)(off + size)};
  }
  for (uint32_t k = 1; k < levels; k++)
    for (uint32_t j = 0; j < k; j++)
      if (level[k].overlaps(level[j])) return bad_arg(ctx, entry, name, ": two levels overlap");
  return OXC_OK;
}

}  // namespace

oxc_status oxc_apply_eye_adaptation(oxc_ctx* ctx, const oxc_eye_adaptation_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_eye_adaptation_context)) return fail(ctx, OXC_INVALID_ARG, "apply_eye_adaptation: bad context / struct_size");
  const char* const entry = "apply_eye_adaptation";
  uint64_t pixels;
  uint32_t texel;
  OXC_TRY(post_source(ctx, entry, c->width, c->height, c->source_format, pixels, texel));
  OXC_TRY(post_attachment(ctx, entry, c->final_attachment, pixels, texel));
  if (bad_pixel_buffer(c->histogram_buffer, 256u, 4u)) return bad_arg(ctx, entry, "histogram_buffer must be 256 aligned u32");
  if (bad_pixel_buffer(c->exposure_buffer, 2u, 4u)) return bad_arg(ctx, entry, "exposure_buffer must be two aligned f32");
  const float exposure_range = c->max_exposure - c->min_exposure;
  if (!std::isfinite(c->min_exposure) || !std::isfinite(c->max_exposure) || !std::isfinite(c->ev100_bias) || !std::isfinite(c->time_coeff) || !std::isfinite(exposure_range))
    return bad_arg(ctx, entry, "min_exposure, max_exposure, ev100_bias, time_coeff and max_exposure - min_exposure must be finite");
  if (!(c->max_exposure > c->min_exposure)) return bad_arg(ctx, entry, "max_exposure must be above min_exposure");
  OXC_ENTER(ctx, hip_stream, s);
  EyeAdaptationArgs a;
  std::memset(&a, 0, sizeof a);
  a.src = c->final_attachment.dptr;
  a.histogram = static_cast<uint32_t*>(c->histogram_buffer.dptr);
  a.exposure = static_cast<float*>(c->exposure_buffer.dptr);
  a.pixels = pixels;
  // the texels before the first 16-byte boundary (the buffer is aligned to its texel), then whole vectors
  const uint32_t per_vector = 16u / texel;
  const uint64_t misaligned = ((16u - (reinterpret_cast<uintptr_t>(a.src) & 15u)) & 15u) / texel;
  a.head = (uint32_t)std::min<uint64_t>(misaligned, pixels);
  a.vectors = (pixels - a.head) / per_vector;
  a.format = c->source_format;
  a.min_exposure = c->min_exposure;
  a.exposure_range = exposure_range;
  a.pixel_count = (float)(uint32_t)pixels;
  a.time_coeff = c->time_coeff;
  a.ev100_bias = c->ev100_bias;
  // about one resident round: four blocks of four waves per CU, every thread with at least one vector
  uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((a.vectors + 255u) / 256u, 1u), (uint64_t)ctx->num_cus * 4u);
  if (ctx->eye_adaptation_grid) grid = std::min(grid, ctx->eye_adaptation_grid);
  launch_eye_adaptation(a, grid, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_apply_bloom(oxc_ctx* ctx, const oxc_bloom_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_bloom_context)) return fail(ctx, OXC_INVALID_ARG, "apply_bloom: bad context / struct_size");
  const char* const entry = "apply_bloom";
  if (c->width < 2u || c->height < 2u) return bad_arg(ctx, entry, "width and height must be at least 2");
  const uint32_t w2 = c->width / 2u, h2 = c->height / 2u;
  if (std::max(w2, h2) >= 8192u) return bad_arg(ctx, entry, "extent too large: max(width, height) / 2 must be below 8192 (13 levels)");
  uint32_t levels = 0;  // floor(log2(max(w2, h2))) + 1
  for (uint32_t m = std::max(w2, h2); m; m >>= 1) levels++;
  uint32_t texel;
  OXC_TRY(post_format(ctx, entry, c->source_format, texel));
  const uint64_t pixels = (uint64_t)c->width * c->height;
  OXC_TRY(post_attachment(ctx, entry, c->final_attachment, pixels, texel));
  ByteSpan down[13], up[13];
  OXC_TRY(bloom_pyramid(ctx, entry, c->bloom_downsampled_attachment, "bloom_downsampled_attachment", w2, h2, levels, texel, down));
  OXC_TRY(bloom_pyramid(ctx, entry, c->bloom_upsampled_attachment, "bloom_upsampled_attachment", w2, h2, levels, texel, up));
  const uintptr_t src_lo = reinterpret_cast<uintptr_t>(c->final_attachment.dptr);
  const ByteSpan src = {src_lo, src_lo + (uintptr_t)(pixels * texel)};
  for (uint32_t k = 0; k < levels; k++) {
    if (down[k].overlaps(src) || up[k].overlaps(src)) return bad_arg(ctx, entry, "the two pyramids and final_attachment must not overlap");
    for (uint32_t j = 0; j < levels; j++)
      if (down[k].overlaps(up[j])) return bad_arg(ctx, entry, "the two pyramids and final_attachment must not overlap");
  }
  const bool has_exposure = (c->scene_flags & OXC_SCENE_HAS_EYE_ADAPTATION) != 0u;
  if (has_exposure && bad_pixel_buffer(c->exposure_buffer, 2u, 4u)) return bad_arg(ctx, entry, "exposure_buffer must be two aligned f32");
  if (!std::isfinite(c->threshold) || !std::isfinite(c->soft_threshold) || !std::isfinite(c->clamp_value) || !std::isfinite(c->radius))
    return bad_arg(ctx, entry, "threshold, soft_threshold, clamp_value and radius must be finite");
  OXC_ENTER(ctx, hip_stream, s);
  BloomArgs a;
  std::memset(&a, 0, sizeof a);
  a.src = c->final_attachment.dptr;
  a.exposure = has_exposure ? static_cast<const float*>(c->exposure_buffer.dptr) : nullptr;
  for (uint32_t k = 0; k < levels; k++) {
    a.down[k] = static_cast<char*>(c->bloom_downsampled_attachment.dptr) + c->bloom_downsampled_attachment.level_offset[k];
    a.up[k] = static_cast<char*>(c->bloom_upsampled_attachment.dptr) + c->bloom_upsampled_attachment.level_offset[k];
  }
  a.w = c->width, a.h = c->height, a.w2 = w2, a.h2 = h2;
  a.levels = levels;
  a.tail = ctx->bloom_tail_level ? std::min(std::max(ctx->bloom_tail_level, bloom_lowest_tail(w2, h2, levels)), levels) : bloom_default_tail(w2, h2, levels);
  a.format = c->source_format;
  a.threshold = c->threshold, a.soft_threshold = c->soft_threshold, a.clamp_value = c->clamp_value, a.radius = c->radius;
  launch_bloom(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_apply_tonemap(oxc_ctx* ctx, const oxc_tonemap_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_tonemap_context)) return fail(ctx, OXC_INVALID_ARG, "apply_tonemap: bad context / struct_size");
  const char* const entry = "apply_tonemap";
  const uint32_t flags = c->scene_flags;
  const bool has_exposure = (flags & OXC_SCENE_HAS_EYE_ADAPTATION) != 0u, has_bloom = (flags & OXC_SCENE_HAS_BLOOM) != 0u;
  const bool has_ca = (flags & OXC_SCENE_HAS_CHROMATIC_ABERRATION) != 0u, has_vignette = (flags & OXC_SCENE_HAS_VIGNETTE) != 0u;
  const bool has_grain = (flags & OXC_SCENE_HAS_FILM_GRAIN) != 0u;
  uint64_t pixels;
  uint32_t texel;
  OXC_TRY(post_source(ctx, entry, c->width, c->height, c->source_format, pixels, texel));
  if (c->output_format > 2u) return bad_arg(ctx, entry, "output_format must be 0 (R8G8B8A8 Srgb), 1 (B8G8R8A8 Srgb) or 2 (R8G8B8A8 Unorm)");
  if (c->tonemap_type > 3u) return bad_arg(ctx, entry, "tonemap_type must be 0 (None), 1 (ACES), 2 (AgX) or 3 (GT7)");
  OXC_TRY(post_attachment(ctx, entry, c->final_attachment, pixels, texel));
  if (bad_pixel_buffer(c->dst_attachment, pixels, 4u)) return bad_arg(ctx, entry, "dst_attachment must be one aligned u32 per pixel");
  const oxc_image_pyramid& p = c->bloom_upsampled_attachment;
  const uint32_t bw = c->width / 2u, bh = c->height / 2u;
  if (has_bloom) {
    if (c->width < 2u || c->height < 2u) return bad_arg(ctx, entry, "HasBloom: width and height must be at least 2");
    if (p.width != bw || p.height != bh || p.levels < 1u || p.levels > 13u)
      return bad_arg(ctx, entry, "bloom_upsampled_attachment must have width / 2, height / 2 and at least one level");
    const uint64_t size = (uint64_t)bw * bh * texel, off = p.level_offset[0];
    if (!p.dptr || ((reinterpret_cast<uintptr_t>(p.dptr) + off) & (texel - 1u)) || off > p.bytes || size > p.bytes - off)
      return bad_arg(ctx, entry, "bloom_upsampled_attachment: level 0 must be aligned to its texel and lie inside the allocation");
  }
  const uintptr_t dst_lo = reinterpret_cast<uintptr_t>(c->dst_attachment.dptr);
  const ByteSpan dst = {dst_lo, dst_lo + (uintptr_t)(pixels * 4u)};
  const uintptr_t src_lo = reinterpret_cast<uintptr_t>(c->final_attachment.dptr);
  bool shared = dst.overlaps({src_lo, src_lo + (uintptr_t)(pixels * texel)});
  if (has_bloom) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p.dptr) + (uintptr_t)p.level_offset[0];
    shared = shared || dst.overlaps({lo, lo + (uintptr_t)((uint64_t)bw * bh * texel)});
  }
  if (has_exposure && c->exposure_buffer.dptr) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(c->exposure_buffer.dptr);
    shared = shared || dst.overlaps({lo, lo + 8u});
  }
  if (shared) return bad_arg(ctx, entry, "dst_attachment must not overlap final_attachment, level 0 of bloom_upsampled_attachment or exposure_buffer");
  if (has_exposure && bad_pixel_buffer(c->exposure_buffer, 2u, 4u)) return bad_arg(ctx, entry, "exposure_buffer must be two aligned f32");
  if ((!has_exposure && !std::isfinite(c->exposure)) || (has_bloom && !std::isfinite(c->bloom_intensity)) || (has_ca && !std::isfinite(c->chromatic_aberration_amount)) ||
      (has_vignette && !std::isfinite(c->vignette_amount)) || (has_grain && (!std::isfinite(c->film_grain_scale) || !std::isfinite(c->film_grain_amount))))
    return bad_arg(ctx, entry, "every setting the scene flags read must be finite");
  if (has_grain && !(c->film_grain_scale > 0.0f)) return bad_arg(ctx, entry, "film_grain_scale must be above 0");
  OXC_ENTER(ctx, hip_stream, s);
  TonemapArgs a;
  std::memset(&a, 0, sizeof a);
  a.src = c->final_attachment.dptr;
  a.bloom = has_bloom ? static_cast<const char*>(p.dptr) + p.level_offset[0] : nullptr;
  a.exposure = has_exposure ? static_cast<const float*>(c->exposure_buffer.dptr) : nullptr;
  a.dst = static_cast<uint32_t*>(c->dst_attachment.dptr);
  a.w = c->width, a.h = c->height, a.bw = bw, a.bh = bh;
  a.flags = flags, a.format = c->source_format, a.output_format = c->output_format, a.tonemap_type = c->tonemap_type;
  a.exposure_setting = c->exposure;
  a.vignette_amount = c->vignette_amount;
  a.grain_scale = c->film_grain_scale, a.grain_amount = c->film_grain_amount, a.grain_seed = c->film_grain_seed;
  a.bloom_intensity = c->bloom_intensity;
  if (has_grain) {  // step 9: the saturating truncation of film_grain_scale / 8.0f, 0 taken as 1
    const float q = c->film_grain_scale / 8.0f;
    a.grain_divisor = q >= 2147483648.0f ? 0x7FFFFFFFu : (uint32_t)(int32_t)q;
  }
  if (a.grain_divisor == 0u) a.grain_divisor = 1u;
  tonemap_constants(has_ca ? c->chromatic_aberration_amount : 0.0f, a.k);  // step 5
  launch_tonemap(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_apply_fxaa(oxc_ctx* ctx, const oxc_fxaa_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_fxaa_context)) return fail(ctx, OXC_INVALID_ARG, "apply_fxaa: bad context / struct_size");
  const char* const entry = "apply_fxaa";
  uint64_t pixels;
  uint32_t texel;
  OXC_TRY(post_source(ctx, entry, c->width, c->height, c->source_format, pixels, texel));
  OXC_TRY(post_attachment(ctx, entry, c->final_attachment, pixels, texel));
  OXC_TRY(post_attachment(ctx, entry, c->fxaa_attachment, pixels, texel, "fxaa_attachment"));
  const uintptr_t src_lo = reinterpret_cast<uintptr_t>(c->final_attachment.dptr), dst_lo = reinterpret_cast<uintptr_t>(c->fxaa_attachment.dptr);
  if (ByteSpan{dst_lo, dst_lo + (uintptr_t)(pixels * texel)}.overlaps({src_lo, src_lo + (uintptr_t)(pixels * texel)}))
    return bad_arg(ctx, entry, "fxaa_attachment must not overlap final_attachment");
  OXC_ENTER(ctx, hip_stream, s);
  FxaaArgs a;
  std::memset(&a, 0, sizeof a);
  a.src = c->final_attachment.dptr;
  a.dst = c->fxaa_attachment.dptr;
  a.w = c->width, a.h = c->height, a.format = c->source_format;
  OXC_TRY(arm_counters(ctx, entry, "hipMalloc(fxaa counters)", ctx->fxaa_stats, 16, s, &a.stats));
  launch_fxaa(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_generate_sky_luts(oxc_ctx* ctx, const oxc_sky_lut_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_sky_lut_context)) return fail(ctx, OXC_INVALID_ARG, "generate_sky_luts: bad context / struct_size");
  const char* const entry = "generate_sky_luts";
  const oxc_atmosphere& A = c->atmosphere;
  if (bad_lut_side(A.transmittance_lut_size)) return bad_arg(ctx, entry, "transmittance_lut_size: every side must be in 2 .. 4096");
  if (bad_lut_side(A.multiscattering_lut_size)) return bad_arg(ctx, entry, "multiscattering_lut_size: every side must be in 2 .. 4096");
  OXC_TRY(check_radii(ctx, entry, A));
  OXC_TRY(check_sky_buffers(ctx, entry, {{c->hemisphere_directions, 768u, "hemisphere_directions", false},
                                         {c->sky_transmittance_lut, lut_bytes(A.transmittance_lut_size), "sky_transmittance_lut", true},
                                         {c->sky_multiscatter_lut, lut_bytes(A.multiscattering_lut_size), "sky_multiscatter_lut", true}}));
  OXC_ENTER(ctx, hip_stream, s);
  SkyLutArgs a;
  std::memset(&a, 0, sizeof a);
  a.in.atm = A;
  atmosphere_constants(A, nullptr, a.in.k);
  a.hemisphere = static_cast<const float*>(c->hemisphere_directions.dptr);
  a.transmittance = static_cast<uint2*>(c->sky_transmittance_lut.dptr);
  a.multiscatter = static_cast<uint2*>(c->sky_multiscatter_lut.dptr);
  a.in.transmittance = a.transmittance;
  a.in.multiscatter = a.transmittance;  // the Slang binds the transmittance LUT in the multiscattering image's place
  launch_sky_luts(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_draw_atmosphere(oxc_ctx* ctx, const oxc_atmosphere_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_atmosphere_context)) return fail(ctx, OXC_INVALID_ARG, "draw_atmosphere: bad context / struct_size");
  const char* const entry = "draw_atmosphere";
  const oxc_atmosphere& A = c->atmosphere;
  if (bad_lut_side(A.transmittance_lut_size)) return bad_arg(ctx, entry, "transmittance_lut_size: every side must be in 2 .. 4096");
  if (bad_lut_side(A.multiscattering_lut_size)) return bad_arg(ctx, entry, "multiscattering_lut_size: every side must be in 2 .. 4096");
  if (bad_lut_side(A.sky_view_lut_size)) return bad_arg(ctx, entry, "sky_view_lut_size: every side must be in 2 .. 4096");
  uint64_t aerial_texels;
  OXC_TRY(check_aerial_size(ctx, entry, A.aerial_perspective_lut_size, aerial_texels));
  OXC_TRY(check_radii(ctx, entry, A));
  OXC_TRY(check_sky_buffers(ctx, entry, {{c->sky_transmittance_lut, lut_bytes(A.transmittance_lut_size), "sky_transmittance_lut", false},
                                         {c->sky_multiscatter_lut, lut_bytes(A.multiscattering_lut_size), "sky_multiscatter_lut", false},
                                         {c->sky_view_lut, lut_bytes(A.sky_view_lut_size), "sky_view_lut", true},
                                         {c->sky_aerial_perspective_lut, aerial_texels * 8u, "sky_aerial_perspective_lut", true}}));
  OXC_ENTER(ctx, hip_stream, s);
  AtmosphereArgs a;
  std::memset(&a, 0, sizeof a);
  a.in.atm = A;
  atmosphere_constants(A, &c->camera_position[1], a.in.k);
  a.in.transmittance = static_cast<const uint2*>(c->sky_transmittance_lut.dptr);
  a.in.multiscatter = static_cast<const uint2*>(c->sky_multiscatter_lut.dptr);
  std::memcpy(a.sun_dir, c->sun_dir, sizeof a.sun_dir);
  a.sun_intensity = c->sun_intensity;
  std::memcpy(a.camera_position, c->camera_position, sizeof a.camera_position);
  std::memcpy(a.inv_projection_view, c->camera_inv_projection_view, sizeof a.inv_projection_view);
  a.sky_view = static_cast<uint2*>(c->sky_view_lut.dptr);
  a.aerial = static_cast<uint2*>(c->sky_aerial_perspective_lut.dptr);
  launch_atmosphere(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_generate_sky_ibl(oxc_ctx* ctx, const oxc_sky_ibl_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_sky_ibl_context)) return fail(ctx, OXC_INVALID_ARG, "generate_sky_ibl: bad context / struct_size");
  const char* const entry = "generate_sky_ibl";
  const oxc_atmosphere& A = c->atmosphere;
  if (bad_lut_side(A.sky_view_lut_size)) return bad_arg(ctx, entry, "sky_view_lut_size: every side must be in 2 .. 4096");
  if (bad_lut_side(A.transmittance_lut_size)) return bad_arg(ctx, entry, "transmittance_lut_size: every side must be in 2 .. 4096");
  if (c->cube_size < 1u || c->cube_size > 1024u) return bad_arg(ctx, entry, "cube_size must be in 1 .. 1024");
  OXC_TRY(check_radii(ctx, entry, A));
  const uint32_t texels = 6u * c->cube_size * c->cube_size;
  OXC_TRY(check_sky_buffers(ctx, entry, {{c->sky_view_lut, lut_bytes(A.sky_view_lut_size), "sky_view_lut", false},
                                         {c->sky_transmittance_lut, lut_bytes(A.transmittance_lut_size), "sky_transmittance_lut", false},
                                         {c->sky_cubemap, (uint64_t)texels * 8u, "sky_cubemap", true}}));
  OXC_ENTER(ctx, hip_stream, s);
  SkyIblArgs a;
  std::memset(&a, 0, sizeof a);
  a.in.atm = A;
  atmosphere_constants(A, &c->camera_position[1], a.in.k);
  a.in.transmittance = static_cast<const uint2*>(c->sky_transmittance_lut.dptr);
  std::memcpy(a.sun_dir, c->sun_dir, sizeof a.sun_dir);
  a.sun_intensity = c->sun_intensity;
  a.sun_ambient_strength = c->sun_ambient_strength;
  a.frame_index = c->frame_index;
  a.cube_size = c->cube_size;
  a.texels = texels;
  a.sky_view = static_cast<const uint2*>(c->sky_view_lut.dptr);
  a.cube = static_cast<uint2*>(c->sky_cubemap.dptr);
  launch_sky_ibl(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_debug_fxaa_stats(oxc_ctx* ctx, uint32_t* host_out4, void* hip_stream) {
  return read_counters(ctx, "debug_fxaa_stats", "oxc_apply_fxaa", &oxc_ctx::fxaa_stats, host_out4, 16, hip_stream);
}

}  // extern "C"
