// shim_terrain_draw <dir>: runs one terrain draw through RendererInstance::draw_terrain_for_visbuffer of RendererInstance.hpp, with
// projection_scale from RendererInstance::terrain_projection_scale.  Reads <dir>/params.bin (Params below) and the heightmap, the patch
// list, the indirect command and the image before the call, <dir>/<name>.bin, and writes the image and its two resolves as <dir>/<name>.out.
// tests/test_gpu_terrain_draw_shim.py compares them with the Python path's bytes.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  uint32_t width, height, clear, visible_count;
  float projection_view[16];
  float camera_position[3], near_clip;
  double resolution_y, fov_degrees;
  GPU::TerrainData terrain;
  uint32_t map_resolution[2];
  uint32_t pad;
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_terrain_draw", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const size_t pixels = (size_t)p.width * p.height, texels = (size_t)p.map_resolution[0] * p.map_resolution[1];
    RendererInstance self(0);
    const auto load = [&](const char* name, size_t bytes) { return device_buffer(bytes, no_fill, dir + "/" + name + ".bin"); };
    oxc_terrain_draw_context c = {};
    c.clear = p.clear, c.width = p.width, c.height = p.height;
    for (int k = 0; k < 16; k++) c.projection_view[k] = p.projection_view[k];
    for (int k = 0; k < 3; k++) c.camera_position[k] = p.camera_position[k];
    c.near_clip = p.near_clip;
    c.projection_scale = RendererInstance::terrain_projection_scale(p.resolution_y, p.fov_degrees);
    c.terrain = p.terrain;
    c.map_resolution[0] = p.map_resolution[0], c.map_resolution[1] = p.map_resolution[1];
    c.heightmap = load("heightmap", texels * 2u);
    c.visible_patches_buffer = load("visible", (size_t)p.visible_count * 4u);
    c.draw_cmd_buffer = load("draw_cmd", 16u);
    c.visdepth_buffer = load("visdepth", pixels * 8u);
    const Buffer depth = device_buffer(pixels * 4u, 0xEE), vis = device_buffer(pixels * 4u, 0xEE);
    c.depth_attachment.dptr = depth.dptr;
    c.depth_attachment.width = p.width, c.depth_attachment.height = p.height, c.depth_attachment.levels = 1;
    c.visbuffer_attachment = vis;
    self.draw_terrain_for_visbuffer(c);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the pass failed");
    write_out(dir + "/visdepth.out", c.visdepth_buffer);
    write_out(dir + "/depth.out", depth);
    write_out(dir + "/vis.out", vis);
    std::printf("terrain draw ok %.9g\n", (double)c.projection_scale);
  });
}
