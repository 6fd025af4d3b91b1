// Compile-and-link check of the C++ shim: the call sequence of RendererInstance::render's 3D
// pass (Oxylus/src/Render/RendererInstance.cpp:783-884) written against ox::amd.  Built by
// tests/test_abi.py with g++ against liboxcull.so; it is only RUN on a GPU box.
#include <cstdio>

#include "RendererInstance.hpp"

using namespace ox::amd;

int main(int argc, char**) {
  if (argc < 2) {
    std::puts("shim links (pass any argument on a GPU box to create a context)");
    return 0;
  }
  RendererInstance self(0);
  auto cull_camera = GPU::CullCamera{};
  cull_camera.mesh_instance_count = self.prepared_frame.mesh_instance_count;
  auto cull_geometry_context = CullGeometryContext{.use_hiz = true, .init_cull_meshes = true, .cull_camera = cull_camera};
  auto main_geometry_context = MainGeometryContext{.cull_camera = cull_camera};
  const auto run_geometry_pass = [&](bool late) {
    if (late) {
      cull_geometry_context.cull_flags |= GPU::CullFlag::LatePass;
      cull_geometry_context.init_cull_meshes = false;
      cull_geometry_context.cull_camera = cull_camera;
    }
    cull_geometry_context.hiz_attachment = main_geometry_context.hiz_attachment;
    try {
      self.cull_geometry(cull_geometry_context);
    } catch (const std::exception& e) {
      std::printf("expected (no buffers bound): %s\n", e.what());
    }
    main_geometry_context.draw_geometry_cmd_buffer = cull_geometry_context.draw_geometry_cmd_buffer;
    main_geometry_context.visibility_buffer = cull_geometry_context.visibility_buffer;
  };
  run_geometry_pass(false);
  try {
    self.generate_hiz(main_geometry_context);
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  run_geometry_pass(true);
  try { self.decode_visbuffer(main_geometry_context); } catch (const std::exception& e) { std::printf("expected (no attachments bound): %s\n", e.what()); }  // RendererInstance.cpp:924
  try {  // the same pass with the image and sampler tables: oxc_decode_visbuffer_textured
    oxc_material_sampler linear_repeated = {OXC_FILTER_LINEAR, OXC_ADDRESS_REPEAT, OXC_FILTER_LINEAR, 0};
    self.decode_visbuffer(main_geometry_context, Buffer{}, Buffer{&linear_repeated, sizeof linear_repeated});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:974-985: the shadow term, after draw_virtual_shadowmap
    self.resolve_shadowmap(ShadowResolveContext{});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:990-1020: the second shadow term, after resolve_shadowmap
    self.contact_shadows(ContactShadowsContext{});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:1040-1055: the ambient occlusion term pbr_apply reads
    self.generate_ambient_occlusion(AmbientOcclusionContext{});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:136-251 and :1023-1038: the constructor-time LUT pair, then draw_atmosphere between contact shadows and ambient occlusion
    auto atmosphere_context = AtmosphereContext{};
    self.generate_sky_luts(atmosphere_context);
    self.draw_atmosphere(atmosphere_context);
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp: apply_pbr, the consumer of every image above
    auto pbr_context = PBRContext{.depth_attachment = main_geometry_context.depth_attachment,
                                  .albedo_attachment = main_geometry_context.albedo_attachment,
                                  .normal_attachment = main_geometry_context.normal_attachment,
                                  .emissive_attachment = main_geometry_context.emissive_attachment,
                                  .metallic_roughness_occlusion_attachment = main_geometry_context.metallic_roughness_occlusion_attachment};
    self.gpu_scene_flags = OXC_SCENE_HAS_DIRECTIONAL_LIGHT | OXC_SCENE_HAS_SKY;
    auto final_attachment = self.apply_pbr(pbr_context, Buffer{});
    (void)final_attachment;
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:1225-1255: FXAA between apply_pbr and the eye adaptation; its output becomes final_attachment
    auto post_process_context = PostProcessContext{.extent = {.width = 1920, .height = 1080}, .final_attachment = Buffer{}, .fxaa_attachment = Buffer{}};
    self.apply_fxaa(post_process_context);  // HasFXAA clear: nothing runs
    self.gpu_scene_flags |= OXC_SCENE_HAS_FXAA;
    self.apply_fxaa(post_process_context);
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:1278: the post passes start with the eye adaptation
    auto post_process_context = PostProcessContext{.delta_time = 1.0f / 60.0f, .extent = {.width = 1920, .height = 1080}, .final_attachment = Buffer{}};
    self.gpu_scene_flags |= OXC_SCENE_HAS_EYE_ADAPTATION;
    self.eye_adaptation = {.min_exposure = -11.5f, .max_exposure = 18.0f};
    self.apply_eye_adaptation(post_process_context);
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:1282: bloom behind the eye adaptation, with the engine's cvar defaults
    auto post_process_context = PostProcessContext{.extent = {.width = 1920, .height = 1080}, .final_attachment = Buffer{}, .bloom_upsampled_attachment = ImagePyramid{}};
    self.gpu_scene_flags |= OXC_SCENE_HAS_BLOOM;
    self.apply_bloom(post_process_context, BloomCVars{}, ImagePyramid{});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // the last pass of the frame: the tonemap, with the lens effects on
    auto post_process_context = PostProcessContext{.extent = {.width = 1920, .height = 1080}, .final_attachment = Buffer{}, .bloom_upsampled_attachment = ImagePyramid{},
                                                   .bloom_intensity = BloomCVars{}.intensity, .dst_attachment = Buffer{}};
    self.gpu_scene_flags |= OXC_SCENE_HAS_FILM_GRAIN | OXC_SCENE_HAS_CHROMATIC_ABERRATION | OXC_SCENE_HAS_VIGNETTE;
    self.post_proces_settings = GPU::PostProcessSettings{.exposure = 1.0f, .film_grain_seed = 7};
    self.tonemap_type = GPU::TonemapType::GT7;
    auto dst_attachment = self.apply_tonemap(post_process_context, /*dst_format: B8G8R8A8 Srgb*/ 1);
    (void)dst_attachment;
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:929-952: the terrain decode directly behind the visbuffer decode
    auto terrain_decode_context = TerrainDecodeContext{.renderer = &self, .terrain = GPU::TerrainData{.layer_material_indices = {0, 1, 2, 3}}, .map_resolution = {2048, 2048}};
    decode_terrain(terrain_decode_context);
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:1300-1323: the debug view in place of the final image
    auto debug_context = DebugContext{.overdraw_heatmap_scale = 10.0f, .debug_view = OXC_DEBUG_VIEW_ALBEDO};
    self.prepared_frame.mesh_instance_count = 1;
    self.apply_debug_view(debug_context, Extent3D{.width = 16, .height = 16});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // ViewportPanel.cpp:1439-1556: the editor's pick behind VisBufferEncode, its mask there and its composite behind PostProcessing
    auto picking_context = PickingContext{.picking_texel = {3, 5}};
    (void)self.pick_transform(picking_context, Extent3D{.width = 16, .height = 16});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {
    auto highlight_context = HighlightContext{.terrain_transform_index = 7, .outline_width = 5, .occluded_mode = 2};
    self.apply_highlight(highlight_context, OXC_HIGHLIGHT_MASK, Extent3D{.width = 16, .height = 16});
    (void)self.apply_highlight(highlight_context, OXC_HIGHLIGHT_COMPOSITE, Extent3D{.width = 16, .height = 16}, Buffer{}, /*dst_format*/ 1);
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // RendererInstance.cpp:1080-1223: the 2D block between apply_pbr and the FXAA pass, and the editor's mouse_picking_2d behind it
    auto sprite_context = SpriteContext{.batch_offset = 0, .batch_count = 4};
    (void)self.draw_sprites(sprite_context, OXC_SPRITES_VIS | OXC_SPRITES_COLOR, Extent3D{.width = 16, .height = 16}, ImageAttachment{}, Buffer{}, /*source_format*/ 0);
    auto sprite_picking = SpritePickingContext{.picking_texel = {3, 5}};
    (void)self.pick_sprite(sprite_picking, Extent3D{.width = 16, .height = 16});
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  try {  // Passes/Terrain.cpp:218-277: the tessellated terrain draw behind draw_for_visbuffer
    oxc_terrain_draw_context terrain_draw = {};
    terrain_draw.width = terrain_draw.height = 16;
    terrain_draw.projection_scale = RendererInstance::terrain_projection_scale(16.0, 60.0);
    self.draw_terrain_for_visbuffer(terrain_draw);
  } catch (const std::exception& e) {
    std::printf("expected (no attachments bound): %s\n", e.what());
  }
  return 0;
}
