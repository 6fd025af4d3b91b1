// shim_terrain_decode <dir>: runs one terrain decode through ox::amd::decode_terrain of RendererInstance.hpp.  Reads <dir>/params.bin (Params
// below) and the inputs and the four attachments as earlier passes left them, <dir>/<name>.bin, and writes the four attachments as
// <dir>/<name>.out.  tests/test_gpu_terrain_decode_shim.py compares them with the Python path's bytes.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  uint32_t width, height;
  float inv_projection_view[16];
  GPU::TerrainData terrain;
  uint32_t map_resolution[2];
  uint32_t material_count;
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_terrain_decode", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const size_t pixels = (size_t)p.width * p.height, texels = (size_t)p.map_resolution[0] * p.map_resolution[1];
    RendererInstance self(0);
    const auto load = [&](const char* name, size_t bytes) { return device_buffer(bytes, no_fill, dir + "/" + name + ".bin"); };
    TerrainDecodeContext context = {};
    context.renderer = &self;
    context.terrain = p.terrain;
    for (int k = 0; k < 16; k++) context.inv_projection_view[k] = p.inv_projection_view[k];
    context.map_resolution = uvec2{p.map_resolution[0], p.map_resolution[1]};
    context.materials_buffer = load("materials", (size_t)p.material_count * 56u);
    context.material_count = p.material_count;
    context.brush_hit_buffer = load("hit", sizeof(GPU::TerrainBrushHit));
    context.visbuffer_attachment = load("vis", pixels * 4u);
    const Buffer depth = load("depth", pixels * 4u);
    context.depth_attachment.dptr = depth.dptr;
    context.depth_attachment.width = p.width, context.depth_attachment.height = p.height, context.depth_attachment.levels = 1;
    context.normalmap_attachment = load("normalmap", texels * 4u);
    context.splatmap_attachment = load("splatmap", texels * 4u);
    context.albedo_attachment = load("albedo", pixels * 4u);
    context.normal_attachment = load("normal", pixels * 8u);
    context.emissive_attachment = load("emissive", pixels * 4u);
    context.metallic_roughness_occlusion_attachment = load("mro", pixels * 4u);
    decode_terrain(context);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the pass failed");
    write_out(dir + "/albedo.out", context.albedo_attachment);
    write_out(dir + "/normal.out", context.normal_attachment);
    write_out(dir + "/emissive.out", context.emissive_attachment);
    write_out(dir + "/mro.out", context.metallic_roughness_occlusion_attachment);
    std::printf("terrain decode ok\n");
  });
}
