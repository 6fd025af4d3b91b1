// shim_terrain_brush <dir>: runs one brush stroke through ox::amd::apply_terrain_brush of RendererInstance.hpp: trace, apply and the three
// regional passes, as RendererInstance::apply_terrain_brush does with painting set.  Reads <dir>/params.bin ({oxc_terrain_brush_params,
// oxc_terrain_generate, oxc_terrain_derive}) and the seven images <dir>/<name>.bin, and writes the images and the two records as
// <dir>/<name>.out.  tests/test_gpu_terrain_brush_shim.py compares them with the Python path's bytes.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  GPU::TerrainBrushParams brush;
  GPU::TerrainGenerate generate;
  GPU::TerrainDerive derive;
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_terrain_brush", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const size_t texels = (size_t)p.brush.resolution[0] * p.brush.resolution[1], patches = (size_t)p.brush.patch_count[0] * p.brush.patch_count[1];
    RendererInstance self(0);
    const struct {
      const char* name;
      size_t bytes;
    } images[] = {{"heightmap", texels * 2u},   {"ridgemap", texels * 2u},   {"normalmap", texels * 4u},   {"splatmap", texels * 4u},
                  {"height_edit", texels * 4u}, {"splat_edit", texels * 4u}, {"patch_minmax", patches * 8u}};
    Buffer b[7];
    for (int k = 0; k < 7; k++) b[k] = device_buffer(images[k].bytes, 0, dir + "/" + images[k].name + ".bin");
    TerrainBrushContext context = {};
    context.maps.renderer = &self;
    context.maps.heightmap = b[0], context.maps.ridgemap = b[1], context.maps.normalmap = b[2], context.maps.splatmap = b[3];
    context.maps.height_edit = b[4], context.maps.splat_edit = b[5];
    context.maps.patch_minmax.dptr = b[6].dptr;
    context.maps.patch_minmax.width = p.brush.patch_count[0], context.maps.patch_minmax.height = p.brush.patch_count[1], context.maps.patch_minmax.levels = 1;
    context.maps.region = device_buffer(sizeof(GPU::TerrainRegion), 0);
    context.hit_buffer = device_buffer(sizeof(GPU::TerrainBrushHit), 0);
    context.params = p.brush;
    context.painting = true;
    context.generate_settings = p.generate;
    context.derive_settings = p.derive;
    apply_terrain_brush(context);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the passes failed");
    for (int k = 0; k < 7; k++) write_out(dir + "/" + images[k].name + ".out", b[k]);
    write_out(dir + "/hit.out", context.hit_buffer.dptr, 16);
    write_out(dir + "/region.out", context.maps.region.dptr, 16);
    std::printf("terrain brush ok\n");
  });
}
