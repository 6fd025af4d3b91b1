// shim_highlight <dir>: runs the editor's selection path through RendererInstance::pick_transform and RendererInstance::apply_highlight of
// RendererInstance.hpp.  Reads <dir>/params.bin (Params below) and the inputs as <dir>/<name>.bin; writes the picked transform as
// <dir>/pick.out, the mask words and the mask image as <dir>/mask_bits.out and <dir>/mask_attachment.out, and the composite of format f in
// mode m as <dir>/dst_format<f>_mode<m>.out.  tests/test_gpu_highlight_shim.py compares them with the golden fixture's bytes.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  uint32_t width, height;
  uint32_t meshlet_instances, mesh_instances, selected;  // record and entry counts
  uint32_t terrain_transform_index;
  uint32_t pick_x, pick_y;
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_highlight", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const size_t pixels = (size_t)p.width * p.height;
    const Extent3D extent = {p.width, p.height, 1};
    RendererInstance self(0);
    const auto load = [&](const char* name, size_t bytes) { return device_buffer(bytes, 0xEE, dir + "/" + name + ".bin"); };
    self.prepared_frame.mesh_instance_count = p.mesh_instances;
    self.prepared_frame.meshlet_instances_buffer = load("meshlet_instances", (size_t)p.meshlet_instances * 8u);
    self.prepared_frame.mesh_instances_buffer = load("mesh_instances", (size_t)p.mesh_instances * 20u);

    PickingContext picking = {};
    picking.picking_texel[0] = p.pick_x, picking.picking_texel[1] = p.pick_y;
    picking.terrain_transform_index = p.terrain_transform_index;
    picking.visbuffer_attachment = load("vis", pixels * 4u);
    picking.transform_id = device_buffer(4u, 0xEE);
    write_out(dir + "/pick.out", self.pick_transform(picking, extent));

    HighlightContext context = {};
    context.transform_indices = load("selected", (size_t)p.selected * 4u);
    context.terrain_transform_index = p.terrain_transform_index;
    context.visbuffer_attachment = picking.visbuffer_attachment;
    context.silhouette_mask_bits = device_buffer((size_t)((p.width + 63u) / 64u) * p.height * 8u, 0xEE);
    context.silhouette_mask = device_buffer(pixels, 0xEE);
    const Buffer depth = load("depth", pixels * 4u);
    context.depth_attachment.dptr = depth.dptr;
    context.depth_attachment.width = p.width, context.depth_attachment.height = p.height, context.depth_attachment.levels = 1;
    context.outlined_composite = device_buffer(pixels * 4u, 0xEE);
    self.apply_highlight(context, OXC_HIGHLIGHT_MASK, extent);
    write_out(dir + "/mask_bits.out", context.silhouette_mask_bits);
    write_out(dir + "/mask_attachment.out", context.silhouette_mask);
    const Buffer color = load("color", pixels * 4u);
    for (uint32_t format = 0; format < 3; format++)
      for (int32_t mode = 0; mode < 3; mode++) {
        if (hipMemset(context.outlined_composite.dptr, 0xEE, pixels * 4u) != hipSuccess) throw std::runtime_error("hipMemset failed");
        context.occluded_mode = mode;
        const Buffer written = self.apply_highlight(context, OXC_HIGHLIGHT_COMPOSITE, extent, color, format);
        write_out(dir + "/dst_format" + std::to_string(format) + "_mode" + std::to_string(mode) + ".out", written);
      }
    std::printf("highlight ok\n");
  });
}
