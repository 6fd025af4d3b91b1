// oxcull_abi_debug.cpp -- the debug views of liboxcull.so's C ABI: oxc_apply_debug_view (the views of the visbuffer, the G-buffer and the VSM
// page table).  Not to be confused with include/oxcull_debug.h, the measurement hooks: this is a pass of the frame.
#include "oxcull_host.hpp"

extern "C" {

oxc_status oxc_apply_debug_view(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_debug_view_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_debug_view_context)) return fail(ctx, OXC_INVALID_ARG, "apply_debug_view: bad context / struct_size");
  const char* const entry = "apply_debug_view";
  const uint32_t view = c->debug_view;
  if (view < OXC_DEBUG_VIEW_TRIANGLES || view > OXC_DEBUG_VIEW_RMVSM) return bad_arg(ctx, entry, "debug_view must be OXC_DEBUG_VIEW_TRIANGLES .. OXC_DEBUG_VIEW_RMVSM");
  const oxc_image& dimg = c->depth_attachment;
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (dimg.width != c->width || dimg.height != c->height) return bad_arg(ctx, entry, "depth_attachment extent differs from (width, height)");
  uint64_t pixels;
  OXC_TRY(pixel_images(ctx, entry, dimg, nullptr, nullptr, pixels));
  const bool vsm = view == OXC_DEBUG_VIEW_RMVSM;
  VsmShape sh = {};
  if (vsm) OXC_TRY(vsm_shape(ctx, entry, *c, sh));
  const bool records = view == OXC_DEBUG_VIEW_MATERIALS || view == OXC_DEBUG_VIEW_MESH_INSTANCES || view == OXC_DEBUG_VIEW_MESH_LODS;
  if (records && !f) return bad_arg(ctx, entry, "the frame must not be null for the Materials, MeshInstances and MeshLods views");

  const uint32_t bit = 1u << view, main_views = 0x7FFEu, rm = 1u << OXC_DEBUG_VIEW_RMVSM;
  const auto on = [](uint32_t v) { return 1u << v; };
  const uint32_t record_views = on(OXC_DEBUG_VIEW_MATERIALS) | on(OXC_DEBUG_VIEW_MESH_INSTANCES) | on(OXC_DEBUG_VIEW_MESH_LODS);
  const oxc_buffer none = {nullptr, 0};
  const oxc_buffer &mli = records ? f->meshlet_instances_buffer : none, &mi = records ? f->mesh_instances_buffer : none, &meshes = records ? f->meshes_buffer : none;
  const oxc_buffer& mro = c->metallic_roughness_occlusion_attachment;
  const MapBuffer buffers[] = {
      {"visbuffer_attachment", c->visbuffer_attachment.dptr, c->visbuffer_attachment.bytes, pixels * 4u, 4u, main_views, 0u, false},
      {"depth_attachment", dimg.dptr, pixels * 4u, pixels * 4u, 4u, main_views | rm, 0u, false},
      {"overdraw_attachment", c->overdraw_attachment.dptr, c->overdraw_attachment.bytes, pixels * 4u, 4u, on(OXC_DEBUG_VIEW_OVERDRAW), 0u, false},
      {"albedo_attachment", c->albedo_attachment.dptr, c->albedo_attachment.bytes, pixels * 4u, 4u, on(OXC_DEBUG_VIEW_ALBEDO), 0u, false},
      {"normal_attachment", c->normal_attachment.dptr, c->normal_attachment.bytes, pixels * 8u, 8u, on(OXC_DEBUG_VIEW_NORMAL) | on(OXC_DEBUG_VIEW_GEOMETRIC_NORMAL), 0u, false},
      {"emissive_attachment", c->emissive_attachment.dptr, c->emissive_attachment.bytes, pixels * 4u, 4u, on(OXC_DEBUG_VIEW_EMISSIVE), 0u, false},
      {"metallic_roughness_occlusion_attachment", mro.dptr, mro.bytes, pixels * 4u, 4u,
       on(OXC_DEBUG_VIEW_METALLIC) | on(OXC_DEBUG_VIEW_ROUGHNESS) | on(OXC_DEBUG_VIEW_BAKED_OCCLUSION), 0u, false},
      {"ambient_occlusion_attachment", c->ambient_occlusion_attachment.dptr, c->ambient_occlusion_attachment.bytes, pixels * 2u, 2u, on(OXC_DEBUG_VIEW_GTAO), 0u, false},
      {"vsm_clipmaps_buffer", c->vsm_clipmaps_buffer.dptr, c->vsm_clipmaps_buffer.bytes, (uint64_t)sh.layers * sizeof(oxc_virtual_clipmap), 4u, rm, 0u, false,
       " is smaller than clipmap_count records"},
      {"virtual_page_table", c->virtual_page_table.dptr, c->virtual_page_table.bytes, sh.entries * 4u, 4u, rm, 0u, false, " is smaller than clipmap_count * n * n u32"},
      {"meshlet_instances_buffer", mli.dptr, mli.bytes, (uint64_t)c->meshlet_instance_count * sizeof(GpuMeshletInstance), 4u, record_views, 0u, false,
       " is smaller than meshlet_instance_count records"},
      {"mesh_instances_buffer", mi.dptr, mi.bytes, mi.bytes, 4u, record_views, 0u, false},
      {"meshes_buffer", meshes.dptr, meshes.bytes, meshes.bytes, 8u, record_views, 0u, false},
      {"debug_attachment", c->debug_attachment.dptr, c->debug_attachment.bytes, pixels * 8u, 8u, main_views | rm, main_views | rm, false},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, bit)) return st;

  OXC_ENTER(ctx, hip_stream, s);
  if (vsm) {
    DebugViewVsmArgs a;
    std::memset(&a, 0, sizeof a);
    a.depth = static_cast<const float*>(dimg.dptr);
    a.out = static_cast<uint2*>(c->debug_attachment.dptr);
    a.w = c->width, a.h = c->height;
    a.clipmaps = static_cast<const float*>(c->vsm_clipmaps_buffer.dptr);
    a.page_table = static_cast<const uint32_t*>(c->virtual_page_table.dptr);
    a.n = (uint32_t)sh.n, a.layers = (uint32_t)sh.layers, a.page_size = (uint32_t)sh.ps;
    a.fn = (float)sh.n, a.fphys = (float)sh.phys;
    a.hue_divisor = (float)((uint32_t)sh.layers + 1u);
    for (int k = 0; k < 16; k++) a.inv_pv[k] = c->inv_projection_view[k];
    clipmap_selection_constants(a, *c, sh);
    launch_debug_view_vsm(a, s);
  } else {
    DebugViewArgs a;
    std::memset(&a, 0, sizeof a);
    a.w = c->width, a.h = c->height;
    a.clear = c->clear ? 1u : 0u;
    a.meshlet_instance_count = c->meshlet_instance_count;
    a.heatmap_scale = c->heatmap_scale;
    a.vis = static_cast<const uint32_t*>(c->visbuffer_attachment.dptr);
    a.depth = static_cast<const float*>(dimg.dptr);
    // only what the view reads: a kernel that touched another input would fault on the null instead of reading the caller's memory
    if (view == OXC_DEBUG_VIEW_OVERDRAW) a.overdraw = static_cast<const uint32_t*>(c->overdraw_attachment.dptr);
    if (view == OXC_DEBUG_VIEW_ALBEDO) a.albedo = static_cast<const uint32_t*>(c->albedo_attachment.dptr);
    if (view == OXC_DEBUG_VIEW_NORMAL || view == OXC_DEBUG_VIEW_GEOMETRIC_NORMAL) a.normal = static_cast<const uint2*>(c->normal_attachment.dptr);
    if (view == OXC_DEBUG_VIEW_EMISSIVE) a.emissive = static_cast<const uint32_t*>(c->emissive_attachment.dptr);
    if (view >= OXC_DEBUG_VIEW_METALLIC && view <= OXC_DEBUG_VIEW_BAKED_OCCLUSION) a.mro = static_cast<const uint32_t*>(mro.dptr);
    if (view == OXC_DEBUG_VIEW_GTAO) a.ao = static_cast<const uint16_t*>(c->ambient_occlusion_attachment.dptr);
    if (records) {
      a.meshlet_instances = static_cast<const GpuMeshletInstance*>(mli.dptr);
      a.mesh_instances = static_cast<const GpuMeshInstance*>(mi.dptr);
      a.meshes = static_cast<const GpuMesh*>(meshes.dptr);
    }
    a.out = static_cast<uint2*>(c->debug_attachment.dptr);
    launch_debug_view(view, a, s);
  }
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

}  // extern "C"
