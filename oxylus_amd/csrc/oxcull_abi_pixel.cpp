// oxcull_abi_pixel.cpp -- the per-pixel passes of liboxcull.so's C ABI: contact shadows, ambient occlusion, visbuffer decode, PBR, and
// their stats readers.
#include "oxcull_host.hpp"

extern "C" {

oxc_status oxc_contact_shadows(oxc_ctx* ctx, const oxc_contact_shadows_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_contact_shadows_context)) return fail(ctx, OXC_INVALID_ARG, "contact_shadows: bad context / struct_size");
  const oxc_image& dimg = c->depth_attachment;
  const oxc_image& oimg = c->contact_shadows_attachment;
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, "contact_shadows", dimg, &oimg, "contact_shadows_attachment", pixels));
  if (c->steps < 1u || c->steps > 64u) return fail(ctx, OXC_INVALID_ARG, "contact_shadows: steps must be 1..64");
  if (!(std::isfinite(c->thickness) && c->thickness > 0.0f) || !(std::isfinite(c->shadow_length) && c->shadow_length > 0.0f) ||
      !(std::isfinite(c->near_clip) && c->near_clip > 0.0f))
    return fail(ctx, OXC_INVALID_ARG, "contact_shadows: thickness, shadow_length and near_clip must be finite and > 0");
  const float* sd = c->sun_dir;
  if (!(std::isfinite(sd[0]) && std::isfinite(sd[1]) && std::isfinite(sd[2])) || (sd[0] == 0.0f && sd[1] == 0.0f && sd[2] == 0.0f))
    return fail(ctx, OXC_INVALID_ARG, "contact_shadows: sun_dir must be finite and not zero");
  OXC_ENTER(ctx, hip_stream, s);
  if (!pixels) return OXC_OK;
  ContactShadowsArgs a;
  std::memset(&a, 0, sizeof a);
  OXC_TRY(arm_counters(ctx, "contact_shadows", "hipMalloc(contact shadows counters)", ctx->contact_shadows_stats, 48, s, &a.stats));
  a.depth = static_cast<const float*>(dimg.dptr);
  a.out = static_cast<float*>(oimg.dptr);
  a.w = dimg.width;
  a.h = dimg.height;
  a.fw = (float)dimg.width;
  a.fh = (float)dimg.height;
  a.steps = c->steps;
  // per-call constants, binary32 in the Slang's order (include/oxcull.h)
  for (int k = 0; k < 16; k++) a.inv_pv[k] = c->inv_projection_view[k], a.view[k] = c->view[k], a.proj[k] = c->projection[k];
  const float len = std::sqrt((sd[0] * sd[0] + sd[1] * sd[1]) + sd[2] * sd[2]);  // normalize(sun_dir) * shadow_length
  for (int k = 0; k < 3; k++) a.ray[k] = (sd[k] / len) * c->shadow_length;
  a.depth_thickness = c->thickness * (1.0f / c->near_clip);
  a.one_plus_bias = 1.0f + 0.000002f;
  a.edge_span = 0.3f - 1.0f;
  launch_contact_shadows(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_generate_ambient_occlusion(oxc_ctx* ctx, const oxc_ambient_occlusion_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_ambient_occlusion_context)) return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: bad context / struct_size");
  const oxc_image& dimg = c->depth_attachment;
  const oxc_image& pimg = c->prefiltered_depth;
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, "generate_ambient_occlusion", dimg, nullptr, nullptr, pixels));
  if (pimg.width != dimg.width || pimg.height != dimg.height || pimg.levels != 5 || (pixels && !pimg.dptr))
    return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: prefiltered_depth must have the depth attachment's extent and exactly 5 levels");
  for (int k = 0; k < 5; k++)
    if (pimg.level_offset[k] & 3u) return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: prefiltered_depth level offsets must be multiples of 4");
  if (bad_pixel_buffer(c->normal_attachment, pixels, 8u))
    return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: normal_attachment must be 8-byte aligned u16x4 texels of the depth attachment's extent");
  if (pixels && (!c->hilbert_noise.dptr || c->hilbert_noise.bytes < 64u * 64u * 2u || (reinterpret_cast<uintptr_t>(c->hilbert_noise.dptr) & 1u)))
    return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: hilbert_noise must be u16[64][64]");
  if (bad_pixel_buffer(c->depth_differences, pixels, 4u)) return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: depth_differences must be one aligned u32 per pixel");
  if (bad_pixel_buffer(c->noisy_occlusion, pixels, 2u) || bad_pixel_buffer(c->ambient_occlusion_attachment, pixels, 2u))
    return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: noisy_occlusion and ambient_occlusion_attachment must be one aligned u16 per pixel");
  if (c->slice_count < 1u || c->slice_count > 16u || c->samples_per_slice_side < 1u || c->samples_per_slice_side > 8u)
    return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: slice_count must be 1..16 and samples_per_slice_side 1..8");
  auto positive = [](float v) { return std::isfinite(v) && v > 0.0f; };
  if (!positive(c->thickness) || !positive(c->effect_radius) || !positive(c->final_power) || !positive(c->far_clip))
    return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: thickness, effect_radius, final_power and far_clip must be finite and > 0");
  if (!positive(c->resolution[0]) || !positive(c->resolution[1])) return fail(ctx, OXC_INVALID_ARG, "generate_ambient_occlusion: resolution must be finite and > 0");
  OXC_ENTER(ctx, hip_stream, s);
  if (!pixels) return OXC_OK;
  AmbientOcclusionArgs a;
  std::memset(&a, 0, sizeof a);
  OXC_TRY(arm_counters(ctx, "generate_ambient_occlusion", "hipMalloc(ambient occlusion counters)", ctx->ambient_occlusion_stats, 64, s, &a.stats));
  a.depth = static_cast<const float*>(dimg.dptr);
  a.normal = static_cast<const uint32_t*>(c->normal_attachment.dptr);
  a.hilbert = static_cast<const uint16_t*>(c->hilbert_noise.dptr);
  a.pre = static_cast<float*>(pimg.dptr);
  a.edges = static_cast<uint32_t*>(c->depth_differences.dptr);
  a.noisy = static_cast<uint16_t*>(c->noisy_occlusion.dptr);
  a.out = static_cast<uint16_t*>(c->ambient_occlusion_attachment.dptr);
  a.w = dimg.width;
  a.h = dimg.height;
  for (uint32_t k = 0; k < 5; k++) {
    a.lvl_off[k] = pimg.level_offset[k] / 4u;
    a.lvl_w[k] = std::max(1u, dimg.width >> k);
    a.lvl_h[k] = std::max(1u, dimg.height >> k);
  }
  a.slice_count = c->slice_count;
  a.samples = c->samples_per_slice_side;
  a.noise_add = 288u * (c->noise_index % 64u);
  // per-call constants, binary32 in the order include/oxcull.h states
  auto falloff = [](float r, float& mul, float& add) {
    const float falloff_range = 0.615f * r;
    const float falloff_from = r * (1.0f - 0.615f);
    mul = -1.0f / falloff_range;
    add = falloff_from / falloff_range + 1.0f;
  };
  a.lin_mul = c->projection[14];  // glm projection[3][2]
  a.lin_add = c->projection[10];  // glm projection[2][2]
  falloff((0.75f * 0.5f) * 1.457f, a.pf_mul, a.pf_add);
  const float r = c->effect_radius * 1.457f;
  falloff(r, a.falloff_mul, a.falloff_add);
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 3; col++) a.view3[row * 3 + col] = c->view[col * 4 + row];
  a.p00 = c->projection[0];
  a.p11 = c->projection[5];
  a.res_x = c->resolution[0];
  a.res_y = c->resolution[1];
  a.far_thr = c->far_clip * 0.999f;
  a.thickness = c->thickness;
  a.slice_count_f = (float)c->slice_count;
  a.samples_f = (float)c->samples_per_slice_side;
  const float half_r = 0.5f * r;
  a.radius_x = half_r * std::fabs(a.p00);
  a.radius_y = half_r * std::fabs(a.p11);
  a.final_power = c->final_power;
  launch_ambient_occlusion(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

}  // extern "C"

namespace {
// The limits oxc_decode_visbuffer and oxc_decode_visbuffer_textured share, in the header's order
oxc_status decode_limits(oxc_ctx* ctx, const char* entry, const oxc_prepared_frame* f, const oxc_decode_context* c) {
  const oxc_image& dimg = c->depth_attachment;
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (dimg.width != c->width || dimg.height != c->height) return bad_arg(ctx, entry, "depth_attachment extent differs from the visbuffer's (width, height)");
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, entry, dimg, nullptr, nullptr, pixels));
  if (bad_pixel_buffer(c->visbuffer_attachment, pixels, 4u)) return bad_arg(ctx, entry, "visbuffer_attachment must be one aligned u32 per pixel");
  if (bad_pixel_buffer(c->albedo_attachment, pixels, 4u) || bad_pixel_buffer(c->emissive_attachment, pixels, 4u) ||
      bad_pixel_buffer(c->metallic_roughness_occlusion_attachment, pixels, 4u))
    return bad_arg(ctx, entry, "albedo_attachment, emissive_attachment and metallic_roughness_occlusion_attachment must be one aligned u32 per pixel");
  if (bad_pixel_buffer(c->normal_attachment, pixels, 8u)) return bad_arg(ctx, entry, "normal_attachment must be 8-byte aligned u16x4 texels of the depth attachment's extent");
  const oxc_buffer& mat = c->materials_buffer;
  if (c->material_count && (!mat.dptr || mat.bytes < (uint64_t)c->material_count * 56u || (reinterpret_cast<uintptr_t>(mat.dptr) & 3u)))
    return bad_arg(ctx, entry, "materials_buffer must hold material_count 4-byte aligned GPU::Material records of 56 bytes");
  if (!f->meshes_buffer.dptr || !f->transforms_world_buffer.dptr || !f->mesh_instances_buffer.dptr || !f->meshlet_instances_buffer.dptr)
    return bad_arg(ctx, entry, "null PreparedFrame buffer");
  if (f->meshlet_instances_buffer.bytes < (uint64_t)c->meshlet_instance_count * sizeof(GpuMeshletInstance))
    return bad_arg(ctx, entry, "meshlet_instances_buffer smaller than meshlet_instance_count records");
  if (reinterpret_cast<uintptr_t>(f->transforms_world_buffer.dptr) & 15u) return bad_arg(ctx, entry, "transforms_world_buffer must be 16-byte aligned");
  return OXC_OK;
}

// The kernel arguments both calls take from the frame and the context (`a` zeroed; stats set by the caller)
void decode_args(const oxc_prepared_frame* f, const oxc_decode_context* c, VisbufferDecodeArgs& a) {
  const oxc_image& dimg = c->depth_attachment;
  const oxc_buffer& mat = c->materials_buffer;
  a.vis = static_cast<const uint32_t*>(c->visbuffer_attachment.dptr);
  a.depth_bits = static_cast<const uint32_t*>(dimg.dptr);
  a.albedo = static_cast<uint32_t*>(c->albedo_attachment.dptr);
  a.normal = static_cast<uint2*>(c->normal_attachment.dptr);
  a.emissive = static_cast<uint32_t*>(c->emissive_attachment.dptr);
  a.mro = static_cast<uint32_t*>(c->metallic_roughness_occlusion_attachment.dptr);
  a.w = c->width;
  a.h = c->height;
  a.fw = (float)c->width;
  a.fh = (float)c->height;
  a.clear = c->clear ? 1u : 0u;
  a.meshlet_instance_count = c->meshlet_instance_count;
  a.material_count = c->material_count;
  a.meshlet_instances = static_cast<const GpuMeshletInstance*>(f->meshlet_instances_buffer.dptr);
  a.mesh_instances = static_cast<const GpuMeshInstance*>(f->mesh_instances_buffer.dptr);
  a.meshes = static_cast<const GpuMesh*>(f->meshes_buffer.dptr);
  a.transforms = static_cast<const float*>(f->transforms_world_buffer.dptr);
  a.materials = static_cast<const uint32_t*>(mat.dptr);
  for (int k = 0; k < 16; k++) a.pv[k] = c->projection_view[k];
}
}  // namespace

extern "C" {

oxc_status oxc_decode_visbuffer(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_decode_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!f || !c || c->struct_size != sizeof(oxc_decode_context)) return fail(ctx, OXC_INVALID_ARG, "decode_visbuffer: bad frame / context / struct_size");
  const char* const entry = "decode_visbuffer";
  OXC_TRY(decode_limits(ctx, entry, f, c));
  OXC_ENTER(ctx, hip_stream, s);
  VisbufferDecodeArgs a;
  std::memset(&a, 0, sizeof a);
  OXC_TRY(arm_counters(ctx, entry, "hipMalloc(visbuffer decode counters)", ctx->visbuffer_decode_stats, 16, s, &a.stats));
  decode_args(f, c, a);
  launch_visbuffer_decode(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_decode_visbuffer_textured(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_decode_context* c, const oxc_material_images* m, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!f || !c || !m || c->struct_size != sizeof(oxc_decode_context) || m->struct_size != sizeof(oxc_material_images))
    return fail(ctx, OXC_INVALID_ARG, "decode_visbuffer_textured: bad frame / context / images / struct_size");
  const char* const entry = "decode_visbuffer_textured";
  OXC_TRY(decode_limits(ctx, entry, f, c));
  const oxc_buffer& img = m->images_buffer;
  if (m->image_count && (!img.dptr || img.bytes < (uint64_t)m->image_count * sizeof(oxc_material_image) || (reinterpret_cast<uintptr_t>(img.dptr) & 7u)))
    return bad_arg(ctx, entry, "images_buffer must hold image_count 8-byte aligned oxc_material_image records of 144 bytes");
  const oxc_buffer& smp = m->samplers_buffer;
  if (m->sampler_count && (!smp.dptr || smp.bytes < (uint64_t)m->sampler_count * sizeof(oxc_material_sampler) || (reinterpret_cast<uintptr_t>(smp.dptr) & 3u)))
    return bad_arg(ctx, entry, "samplers_buffer must hold sampler_count 4-byte aligned oxc_material_sampler records of 16 bytes");
  OXC_ENTER(ctx, hip_stream, s);
  VisbufferDecodeTexturedArgs a;
  std::memset(&a, 0, sizeof a);
  OXC_TRY(arm_counters(ctx, entry, "hipMalloc(textured visbuffer decode counters)", ctx->visbuffer_decode_textured_stats, 64, s, &a.g.stats));
  decode_args(f, c, a.g);
  for (int k = 0; k < 3; k++) a.camera_position[k] = m->camera_position[k];
  a.image_count = m->image_count;
  a.sampler_count = m->sampler_count;
  a.images = m->image_count ? static_cast<const MaterialImage*>(img.dptr) : nullptr;
  a.samplers = m->sampler_count ? static_cast<const uint32_t*>(smp.dptr) : nullptr;
  launch_visbuffer_decode_textured(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_apply_pbr(oxc_ctx* ctx, const oxc_pbr_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_pbr_context)) return fail(ctx, OXC_INVALID_ARG, "apply_pbr: bad context / struct_size");
  const char* const entry = "apply_pbr";
  const oxc_image& dimg = c->depth_attachment;
  const uint32_t flags = c->scene_flags;
  if (flags & OXC_SCENE_HAS_ATMOSPHERE) return bad_arg(ctx, entry, "HasAtmosphere: the atmosphere branch (pbr_apply.slang) is oxc_apply_pbr_atmosphere, not this call");
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (dimg.width != c->width || dimg.height != c->height) return bad_arg(ctx, entry, "depth_attachment extent differs from (width, height)");
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, entry, dimg, (flags & OXC_SCENE_HAS_DIRECTIONAL_LIGHT) ? &c->resolved_shadows_attachment : nullptr, "resolved_shadows_attachment", pixels));
  OXC_TRY(pixel_images(ctx, entry, dimg, (flags & OXC_SCENE_HAS_CONTACT_SHADOWS) ? &c->contact_shadows_attachment : nullptr, "contact_shadows_attachment", pixels));
  if (bad_pixel_buffer(c->albedo_attachment, pixels, 4u) || bad_pixel_buffer(c->emissive_attachment, pixels, 4u) ||
      bad_pixel_buffer(c->metallic_roughness_occlusion_attachment, pixels, 4u))
    return bad_arg(ctx, entry, "albedo_attachment, emissive_attachment and metallic_roughness_occlusion_attachment must be one aligned u32 per pixel");
  if (bad_pixel_buffer(c->normal_attachment, pixels, 8u)) return bad_arg(ctx, entry, "normal_attachment must be 8-byte aligned u16x4 texels of the depth attachment's extent");
  if (bad_pixel_buffer(c->ambient_occlusion_attachment, pixels, 2u)) return bad_arg(ctx, entry, "ambient_occlusion_attachment must be one aligned u16 per pixel");
  const bool transparent = (flags & OXC_SCENE_TRANSPARENT_BACKGROUND) != 0u;
  if (bad_pixel_buffer(c->final_attachment, pixels, transparent ? 8u : 4u))
    return bad_arg(ctx, entry, "final_attachment must be one aligned u32 per pixel, or one 8-byte aligned u16x4 per pixel with TransparentBackground");
  const oxc_buffer& lb = c->lights_buffer;
  if (c->light_count && (!lb.dptr || lb.bytes < (uint64_t)c->light_count * 64u || (reinterpret_cast<uintptr_t>(lb.dptr) & 3u)))
    return bad_arg(ctx, entry, "lights_buffer must hold light_count 4-byte aligned GPU::Light records of 64 bytes");
  bool finite = std::isfinite(c->sun_intensity);
  for (int k = 0; k < 16; k++) finite = finite && std::isfinite(c->inv_projection_view[k]);
  for (int k = 0; k < 3; k++)
    finite = finite && std::isfinite(c->camera_position[k]) && std::isfinite(c->sun_dir[k]) && std::isfinite(c->base_ambient_color[k]) && std::isfinite(c->sky_ambient_color[k]);
  for (int k = 0; k < 4; k++) finite = finite && std::isfinite(c->sky_solid_color[k]);
  if (!finite) return bad_arg(ctx, entry, "inv_projection_view, camera_position, sun_dir, sun_intensity and the three colours must be finite");
  OXC_ENTER(ctx, hip_stream, s);
  PbrApplyArgs a;
  std::memset(&a, 0, sizeof a);
  OXC_TRY(arm_counters(ctx, entry, "hipMalloc(pbr apply counters)", ctx->pbr_apply_stats, 36, s, &a.stats));
  a.depth = static_cast<const float*>(dimg.dptr);
  a.albedo = static_cast<const uint32_t*>(c->albedo_attachment.dptr);
  a.normal = static_cast<const uint2*>(c->normal_attachment.dptr);
  a.emissive = static_cast<const uint32_t*>(c->emissive_attachment.dptr);
  a.mro = static_cast<const uint32_t*>(c->metallic_roughness_occlusion_attachment.dptr);
  a.ao = static_cast<const uint16_t*>(c->ambient_occlusion_attachment.dptr);
  a.resolved = (flags & OXC_SCENE_HAS_DIRECTIONAL_LIGHT) ? static_cast<const float*>(c->resolved_shadows_attachment.dptr) : nullptr;
  a.contact = (flags & OXC_SCENE_HAS_CONTACT_SHADOWS) ? static_cast<const float*>(c->contact_shadows_attachment.dptr) : nullptr;
  a.lights = lb.dptr;
  a.out = c->final_attachment.dptr;
  a.w = c->width;
  a.h = c->height;
  a.fw = (float)c->width;
  a.fh = (float)c->height;
  a.flags = flags;
  a.light_count = c->light_count;
  for (int k = 0; k < 16; k++) a.inv_pv[k] = c->inv_projection_view[k];
  for (int k = 0; k < 3; k++) {
    a.camera[k] = c->camera_position[k], a.sun[k] = c->sun_dir[k];
    a.env[k] = (flags & OXC_SCENE_HAS_SKY) ? c->sky_ambient_color[k] : c->base_ambient_color[k];
    a.sky_color[k] = c->sky_has_texture ? 1.0f : c->sky_solid_color[k];
  }
  a.sun_intensity = c->sun_intensity;
  launch_pbr_apply(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_apply_pbr_atmosphere(oxc_ctx* ctx, const oxc_pbr_atmosphere_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_pbr_atmosphere_context)) return fail(ctx, OXC_INVALID_ARG, "apply_pbr_atmosphere: bad context / struct_size");
  const char* const entry = "apply_pbr_atmosphere";
  const oxc_image& dimg = c->depth_attachment;
  const oxc_atmosphere& A = c->atmosphere;
  const uint32_t flags = c->scene_flags;
  const bool has_sun = (flags & OXC_SCENE_HAS_DIRECTIONAL_LIGHT) != 0u, has_contact = (flags & OXC_SCENE_HAS_CONTACT_SHADOWS) != 0u;
  // 2. the extent
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (dimg.width != c->width || dimg.height != c->height) return bad_arg(ctx, entry, "depth_attachment extent differs from (width, height)");
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, entry, dimg, nullptr, nullptr, pixels));
  // 3 - 8. the record
  if (bad_lut_side(A.transmittance_lut_size)) return bad_arg(ctx, entry, "transmittance_lut_size: every side must be in 2 .. 4096");
  if (bad_lut_side(A.sky_view_lut_size)) return bad_arg(ctx, entry, "sky_view_lut_size: every side must be in 2 .. 4096");
  uint64_t aerial_texels;
  OXC_TRY(check_aerial_size(ctx, entry, A.aerial_perspective_lut_size, aerial_texels));
  if (c->cube_size < 1u || c->cube_size > 1024u) return bad_arg(ctx, entry, "cube_size must be in 1 .. 1024");
  OXC_TRY(check_radii(ctx, entry, A));
  if (!std::isfinite(A.aerial_perspective_start_km) || !std::isfinite(A.aerial_perspective_exposure))
    return bad_arg(ctx, entry, "aerial_perspective_start_km and aerial_perspective_exposure must be finite");
  // 9. the host scalars
  bool finite = std::isfinite(c->sun_intensity);
  for (int k = 0; k < 16; k++) finite = finite && std::isfinite(c->inv_projection_view[k]);
  for (int k = 0; k < 3; k++) finite = finite && std::isfinite(c->camera_position[k]) && std::isfinite(c->sun_dir[k]);
  if (!finite) return bad_arg(ctx, entry, "inv_projection_view, camera_position, sun_dir and sun_intensity must be finite");
  // 10. the G-buffer, the shadow terms, the lights: oxc_apply_pbr's rules
  OXC_TRY(pixel_images(ctx, entry, dimg, has_sun ? &c->resolved_shadows_attachment : nullptr, "resolved_shadows_attachment", pixels));
  OXC_TRY(pixel_images(ctx, entry, dimg, has_contact ? &c->contact_shadows_attachment : nullptr, "contact_shadows_attachment", pixels));
  if (bad_pixel_buffer(c->albedo_attachment, pixels, 4u) || bad_pixel_buffer(c->emissive_attachment, pixels, 4u) ||
      bad_pixel_buffer(c->metallic_roughness_occlusion_attachment, pixels, 4u))
    return bad_arg(ctx, entry, "albedo_attachment, emissive_attachment and metallic_roughness_occlusion_attachment must be one aligned u32 per pixel");
  if (bad_pixel_buffer(c->normal_attachment, pixels, 8u)) return bad_arg(ctx, entry, "normal_attachment must be 8-byte aligned u16x4 texels of the depth attachment's extent");
  if (bad_pixel_buffer(c->ambient_occlusion_attachment, pixels, 2u)) return bad_arg(ctx, entry, "ambient_occlusion_attachment must be one aligned u16 per pixel");
  const oxc_buffer& lb = c->lights_buffer;
  if (c->light_count && (!lb.dptr || lb.bytes < (uint64_t)c->light_count * 64u || (reinterpret_cast<uintptr_t>(lb.dptr) & 3u)))
    return bad_arg(ctx, entry, "lights_buffer must hold light_count 4-byte aligned GPU::Light records of 64 bytes");
  // 11. the four sky images
  const uint64_t t_bytes = lut_bytes(A.transmittance_lut_size), v_bytes = lut_bytes(A.sky_view_lut_size), a_bytes = aerial_texels * 8u,
                 c_bytes = 6ull * c->cube_size * c->cube_size * 8u;
  OXC_TRY(check_sky_buffers(ctx, entry, {{c->sky_transmittance_lut, t_bytes, "sky_transmittance_lut", false},
                                         {c->sky_view_lut, v_bytes, "sky_view_lut", false},
                                         {c->sky_aerial_perspective_lut, a_bytes, "sky_aerial_perspective_lut", false},
                                         {c->sky_cubemap, c_bytes, "sky_cubemap", false}}));
  // 12. the output
  const bool transparent = (flags & OXC_SCENE_TRANSPARENT_BACKGROUND) != 0u;
  const uint64_t texel = transparent ? 8u : 4u;
  if (bad_pixel_buffer(c->final_attachment, pixels, texel))
    return bad_arg(ctx, entry, "final_attachment must be one aligned u32 per pixel, or one 8-byte aligned u16x4 per pixel with TransparentBackground");
  const uintptr_t out_lo = reinterpret_cast<uintptr_t>(c->final_attachment.dptr);
  const ByteSpan out = {out_lo, out_lo + (uintptr_t)(pixels * texel)};
  const struct {
    const void* dptr;
    uint64_t bytes;
    const char* name;
  } inputs[] = {{dimg.dptr, pixels * 4u, "depth_attachment"},
                {c->albedo_attachment.dptr, pixels * 4u, "albedo_attachment"},
                {c->normal_attachment.dptr, pixels * 8u, "normal_attachment"},
                {c->emissive_attachment.dptr, pixels * 4u, "emissive_attachment"},
                {c->metallic_roughness_occlusion_attachment.dptr, pixels * 4u, "metallic_roughness_occlusion_attachment"},
                {c->ambient_occlusion_attachment.dptr, pixels * 2u, "ambient_occlusion_attachment"},
                {has_sun ? c->resolved_shadows_attachment.dptr : nullptr, pixels * 4u, "resolved_shadows_attachment"},
                {has_contact ? c->contact_shadows_attachment.dptr : nullptr, pixels * 4u, "contact_shadows_attachment"},
                {c->light_count ? lb.dptr : nullptr, (uint64_t)c->light_count * 64u, "lights_buffer"},
                {c->sky_transmittance_lut.dptr, t_bytes, "sky_transmittance_lut"},
                {c->sky_view_lut.dptr, v_bytes, "sky_view_lut"},
                {c->sky_aerial_perspective_lut.dptr, a_bytes, "sky_aerial_perspective_lut"},
                {c->sky_cubemap.dptr, c_bytes, "sky_cubemap"}};
  for (const auto& in : inputs) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(in.dptr);
    if (in.dptr && out.overlaps({lo, lo + (uintptr_t)in.bytes})) return bad_arg(ctx, entry, "final_attachment must not overlap ", in.name);
  }
  OXC_ENTER(ctx, hip_stream, s);
  PbrAtmosphereArgs a;
  std::memset(&a, 0, sizeof a);
  PbrApplyArgs& g = a.g;
  g.depth = static_cast<const float*>(dimg.dptr);
  g.albedo = static_cast<const uint32_t*>(c->albedo_attachment.dptr);
  g.normal = static_cast<const uint2*>(c->normal_attachment.dptr);
  g.emissive = static_cast<const uint32_t*>(c->emissive_attachment.dptr);
  g.mro = static_cast<const uint32_t*>(c->metallic_roughness_occlusion_attachment.dptr);
  g.ao = static_cast<const uint16_t*>(c->ambient_occlusion_attachment.dptr);
  g.resolved = has_sun ? static_cast<const float*>(c->resolved_shadows_attachment.dptr) : nullptr;
  g.contact = has_contact ? static_cast<const float*>(c->contact_shadows_attachment.dptr) : nullptr;
  g.lights = lb.dptr;
  g.out = c->final_attachment.dptr;
  g.w = c->width;
  g.h = c->height;
  g.fw = (float)c->width;
  g.fh = (float)c->height;
  g.flags = flags;
  g.light_count = c->light_count;
  for (int k = 0; k < 16; k++) g.inv_pv[k] = c->inv_projection_view[k];
  for (int k = 0; k < 3; k++) g.camera[k] = c->camera_position[k], g.sun[k] = c->sun_dir[k];
  g.sun_intensity = c->sun_intensity;
  a.transmittance = static_cast<const uint2*>(c->sky_transmittance_lut.dptr);
  a.sky_view = static_cast<const uint2*>(c->sky_view_lut.dptr);
  a.aerial = static_cast<const uint2*>(c->sky_aerial_perspective_lut.dptr);
  a.cube = static_cast<const uint2*>(c->sky_cubemap.dptr);
  a.cube_size = c->cube_size;
  AtmosphereConstants k;
  atmosphere_constants(A, &c->camera_position[1], k);
  a.h_atmos = k.h_atmos, a.eye_altitude = k.eye_altitude, a.beta = k.beta, a.zenith_horizon_angle = k.zenith_horizon_angle;
  pbr_atmosphere_constants(A, a);
  launch_pbr_apply_atmosphere(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_debug_contact_shadows_stats(oxc_ctx* ctx, uint32_t* host_out12, void* hip_stream) {
  return read_counters(ctx, "debug_contact_shadows_stats", "oxc_contact_shadows", &oxc_ctx::contact_shadows_stats, host_out12, 48, hip_stream);
}

oxc_status oxc_debug_ambient_occlusion_stats(oxc_ctx* ctx, uint32_t* host_out15, void* hip_stream) {
  return read_counters(ctx, "debug_ambient_occlusion_stats", "oxc_generate_ambient_occlusion", &oxc_ctx::ambient_occlusion_stats, host_out15, 60, hip_stream);
}

oxc_status oxc_debug_visbuffer_decode_stats(oxc_ctx* ctx, uint32_t* host_out4, void* hip_stream) {
  return read_counters(ctx, "debug_visbuffer_decode_stats", "oxc_decode_visbuffer", &oxc_ctx::visbuffer_decode_stats, host_out4, 16, hip_stream);
}

oxc_status oxc_debug_visbuffer_decode_textured_stats(oxc_ctx* ctx, uint32_t* host_out13, void* hip_stream) {
  return read_counters(ctx, "debug_visbuffer_decode_textured_stats", "oxc_decode_visbuffer_textured", &oxc_ctx::visbuffer_decode_textured_stats, host_out13, 52, hip_stream);
}

oxc_status oxc_debug_pbr_apply_stats(oxc_ctx* ctx, uint32_t* host_out9, void* hip_stream) {
  return read_counters(ctx, "debug_pbr_apply_stats", "oxc_apply_pbr", &oxc_ctx::pbr_apply_stats, host_out9, 36, hip_stream);
}

}  // extern "C"
