// oxcull_abi_editor.cpp -- the editor's selection path of liboxcull.so's C ABI: oxc_pick_transform (which transform lies under a texel) and
// oxc_apply_highlight (the selection mask and the outline composite).
#include "oxcull_host.hpp"

namespace {
HighlightRecords records_of(const oxc_prepared_frame& f, const oxc_buffer& vis, uint32_t w, uint32_t h, uint32_t meshlet_instance_count, uint32_t terrain_transform_index) {
  return {static_cast<const uint32_t*>(vis.dptr), static_cast<const GpuMeshletInstance*>(f.meshlet_instances_buffer.dptr),
          static_cast<const GpuMeshInstance*>(f.mesh_instances_buffer.dptr), w, h, meshlet_instance_count, terrain_transform_index};
}
}  // namespace

extern "C" {

oxc_status oxc_pick_transform(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_pick_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_pick_context)) return fail(ctx, OXC_INVALID_ARG, "pick_transform: bad context / struct_size");
  const char* const entry = "pick_transform";
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (c->width > 65536u || c->height > 65536u) return bad_arg(ctx, entry, "extent beyond 65536");
  if (c->x >= c->width || c->y >= c->height) return bad_arg(ctx, entry, "the texel lies outside the image");
  if (!f) return bad_arg(ctx, entry, "the frame must not be null");
  const uint64_t pixels = (uint64_t)c->width * c->height;
  const oxc_buffer &mli = f->meshlet_instances_buffer, &mi = f->mesh_instances_buffer;
  const MapBuffer buffers[] = {
      {"visbuffer_attachment", c->visbuffer_attachment.dptr, c->visbuffer_attachment.bytes, pixels * 4u, 4u, 1u, 0u, false},
      {"transform_id", c->transform_id.dptr, c->transform_id.bytes, 4u, 4u, 1u, 1u, false},
      {"meshlet_instances_buffer", mli.dptr, mli.bytes, (uint64_t)c->meshlet_instance_count * sizeof(GpuMeshletInstance), 4u, 1u, 0u, false,
       " is smaller than meshlet_instance_count records"},
      {"mesh_instances_buffer", mi.dptr, mi.bytes, mi.bytes, 4u, 1u, 0u, false},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, 1u)) return st;

  OXC_ENTER(ctx, hip_stream, s);
  PickArgs a;
  a.r = records_of(*f, c->visbuffer_attachment, c->width, c->height, c->meshlet_instance_count, c->terrain_transform_index);
  a.x = c->x, a.y = c->y;
  a.out = static_cast<uint32_t*>(c->transform_id.dptr);
  launch_pick_transform(a, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_apply_highlight(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_highlight_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_highlight_context)) return fail(ctx, OXC_INVALID_ARG, "apply_highlight: bad context / struct_size");
  const char* const entry = "apply_highlight";
  const uint32_t stages = c->stages, mask = OXC_HIGHLIGHT_MASK, composite = OXC_HIGHLIGHT_COMPOSITE;
  if (stages == 0u || (stages & ~(mask | composite))) return bad_arg(ctx, entry, "stages must be a non-empty set of OXC_HIGHLIGHT_MASK and OXC_HIGHLIGHT_COMPOSITE");
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (c->width > 65536u || c->height > 65536u) return bad_arg(ctx, entry, "extent beyond 65536");
  const oxc_image& dimg = c->depth_attachment;
  const uint32_t rx = (uint32_t)std::max(1, c->dilate_radius), ry = (uint32_t)std::max(1, c->outline_width);  // H1
  if (stages & composite) {
    if (c->color_format > 2u) return bad_arg(ctx, entry, "color_format must be 0, 1 or 2");
    if (rx > 255u || ry > 255u) return bad_arg(ctx, entry, "dilate_radius and outline_width must be at most 255");
    if (dimg.width != c->width || dimg.height != c->height) return bad_arg(ctx, entry, "depth_attachment extent differs from (width, height)");
    if (dimg.levels != 1 || dimg.level_offset[0] != 0) return bad_arg(ctx, entry, "depth_attachment must be one R32F level at offset 0");
  }
  if ((stages & mask) && !f) return bad_arg(ctx, entry, "the frame must not be null for the mask stage");

  const uint64_t pixels = (uint64_t)c->width * c->height, words = (uint64_t)((c->width + 63u) / 64u) * c->height;
  const oxc_buffer none = {nullptr, 0};
  const oxc_buffer &mli = f ? f->meshlet_instances_buffer : none, &mi = f ? f->mesh_instances_buffer : none;
  const MapBuffer buffers[] = {
      {"visbuffer_attachment", c->visbuffer_attachment.dptr, c->visbuffer_attachment.bytes, pixels * 4u, 4u, mask, 0u, false},
      {"transform_indices", c->transform_indices.dptr, c->transform_indices.bytes, (uint64_t)c->selected_count * 4u, 4u, c->selected_count ? mask : 0u, 0u, false,
       " is smaller than selected_count u32"},
      {"mask_bits", c->mask_bits.dptr, c->mask_bits.bytes, words * 8u, 8u, mask | composite, mask, false},
      {"mask_attachment", c->mask_attachment.dptr, c->mask_attachment.bytes, pixels, 1u, mask, mask, true},
      {"depth_attachment", dimg.dptr, pixels * 4u, pixels * 4u, 4u, composite, 0u, false},
      {"color_attachment", c->color_attachment.dptr, c->color_attachment.bytes, pixels * 4u, 4u, composite, 0u, false},
      {"dst_attachment", c->dst_attachment.dptr, c->dst_attachment.bytes, pixels * 4u, 4u, composite, composite, false},
      {"meshlet_instances_buffer", mli.dptr, mli.bytes, (uint64_t)c->meshlet_instance_count * sizeof(GpuMeshletInstance), 4u, mask, 0u, false,
       " is smaller than meshlet_instance_count records"},
      {"mesh_instances_buffer", mi.dptr, mi.bytes, mi.bytes, 4u, mask, 0u, false},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, stages)) return st;

  OXC_ENTER(ctx, hip_stream, s);
  if (stages & mask) {
    HighlightMaskArgs a;
    a.r = records_of(*f, c->visbuffer_attachment, c->width, c->height, c->meshlet_instance_count, c->terrain_transform_index);
    a.selected = c->selected_count ? static_cast<const uint32_t*>(c->transform_indices.dptr) : nullptr;
    a.selected_count = c->selected_count;
    a.mask_bits = static_cast<uint64_t*>(c->mask_bits.dptr);
    a.mask_attachment = static_cast<uint8_t*>(c->mask_attachment.dptr);
    launch_highlight_mask(a, s);
    OXC_HIP(ctx, hipGetLastError());
  }
  if (stages & composite) {
    HighlightCompositeArgs a;
    a.mask_bits = static_cast<const uint64_t*>(c->mask_bits.dptr);
    a.depth = static_cast<const float*>(dimg.dptr);
    a.color = static_cast<const uint32_t*>(c->color_attachment.dptr);
    a.dst = static_cast<uint32_t*>(c->dst_attachment.dptr);
    a.w = c->width, a.h = c->height, a.format = c->color_format;
    a.rx = rx, a.ry = ry;
    a.occluded_mode = c->occluded_mode;
    highlight_outline_linear(c->outline_color, a.outline);
    if (c->color_format == 1u) std::swap(a.outline[0], a.outline[2]);  // the kernel works in the order of the word's bytes: B, G, R, A
    launch_highlight_composite(a, s);
    OXC_HIP(ctx, hipGetLastError());
  }
  return OXC_OK;
}

}  // extern "C"
