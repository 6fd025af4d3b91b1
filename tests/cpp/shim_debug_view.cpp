// shim_debug_view <dir>: runs the fourteen main debug views through RendererInstance::apply_debug_view of RendererInstance.hpp.  Reads
// <dir>/params.bin (Params below), the eight images and the three record buffers as <dir>/<name>.bin, and writes the debug attachment of
// view k as <dir>/view<k>.out.  tests/test_gpu_debug_view_shim.py compares them with the golden fixture's bytes.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  uint32_t width, height;
  uint32_t meshlet_instances, mesh_instances, meshes;  // record counts
  float heatmap_scale;
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_debug_view", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const size_t pixels = (size_t)p.width * p.height;
    RendererInstance self(0);
    const auto load = [&](const char* name, size_t bytes) { return device_buffer(bytes, no_fill, dir + "/" + name + ".bin"); };
    self.prepared_frame.mesh_instance_count = p.mesh_instances;
    self.prepared_frame.meshlet_instances_buffer = load("meshlet_instances", (size_t)p.meshlet_instances * 8u);
    self.prepared_frame.mesh_instances_buffer = load("mesh_instances", (size_t)p.mesh_instances * 20u);
    self.prepared_frame.meshes_buffer = load("meshes", (size_t)p.meshes * 64u);
    DebugContext context = {};
    context.overdraw_heatmap_scale = p.heatmap_scale;
    context.visbuffer_attachment = load("vis", pixels * 4u);
    const Buffer depth = load("depth", pixels * 4u);
    context.depth_attachment.dptr = depth.dptr;
    context.depth_attachment.width = p.width, context.depth_attachment.height = p.height, context.depth_attachment.levels = 1;
    context.overdraw_attachment = load("overdraw", pixels * 4u);
    context.albedo_attachment = load("albedo", pixels * 4u);
    context.normal_attachment = load("normal", pixels * 8u);
    context.emissive_attachment = load("emissive", pixels * 4u);
    context.metallic_roughness_occlusion_attachment = load("mr_occlusion", pixels * 4u);
    context.ambient_occlusion_attachment = load("ao", pixels * 2u);
    context.debug_attachment = device_buffer(pixels * 8u, no_fill);
    for (uint32_t view = OXC_DEBUG_VIEW_TRIANGLES; view <= OXC_DEBUG_VIEW_GEOMETRIC_NORMAL; view++) {
      if (hipMemset(context.debug_attachment.dptr, 0xEE, pixels * 8u) != hipSuccess) throw std::runtime_error("hipMemset failed");
      context.debug_view = view;
      const Buffer written = self.apply_debug_view(context, Extent3D{p.width, p.height, 1});
      if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the pass failed");
      write_out(dir + "/view" + std::to_string(view) + ".out", written);
    }
    std::printf("debug views ok\n");
  });
}
