// shim_terrain_maps <dir>: runs the three terrain passes through the free functions of RendererInstance.hpp, one after the other, as
// Terrain::bake does.  Reads <dir>/params.bin ({oxc_terrain_generate, oxc_terrain_derive, u32 patch_count[2]}; the resolution is the
// settings') and <dir>/height_edit.bin, <dir>/splat_edit.bin, and writes the five images as <dir>/<name>.out.
// tests/test_gpu_terrain_maps_shim.py compares them with the checker.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  GPU::TerrainGenerate generate;
  GPU::TerrainDerive derive;
  uint32_t patch_count[2];
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_terrain_maps", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const uvec2 resolution = {p.generate.resolution[0], p.generate.resolution[1]}, patch_count = {p.patch_count[0], p.patch_count[1]};
    const size_t texels = (size_t)resolution.x * resolution.y, patches = (size_t)patch_count.x * patch_count.y;
    RendererInstance self(0);
    TerrainMaps maps = {};
    maps.renderer = &self;
    maps.heightmap = device_buffer(texels * 2u, 0);
    maps.ridgemap = device_buffer(texels * 2u, 0);
    maps.normalmap = device_buffer(texels * 4u, 0);
    maps.splatmap = device_buffer(texels * 4u, 0);
    maps.height_edit = device_buffer(texels * 4u, 0, dir + "/height_edit.bin");
    maps.splat_edit = device_buffer(texels * 4u, 0, dir + "/splat_edit.bin");
    maps.patch_minmax.dptr = device_buffer(patches * 8u, 0).dptr;
    maps.patch_minmax.width = patch_count.x, maps.patch_minmax.height = patch_count.y, maps.patch_minmax.levels = 1;
    GPU::TerrainMinMax minmax_settings = {};
    minmax_settings.resolution[0] = resolution.x, minmax_settings.resolution[1] = resolution.y;
    minmax_settings.patch_count[0] = patch_count.x, minmax_settings.patch_count[1] = patch_count.y;
    terrain_generate_pass(maps, p.generate, resolution);
    terrain_derive_pass(maps, p.derive, resolution);
    terrain_minmax_pass(maps, minmax_settings, patch_count);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the passes failed");
    write_out(dir + "/heightmap.out", maps.heightmap);
    write_out(dir + "/ridgemap.out", maps.ridgemap);
    write_out(dir + "/normalmap.out", maps.normalmap);
    write_out(dir + "/splatmap.out", maps.splatmap);
    write_out(dir + "/patch_minmax.out", maps.patch_minmax.dptr, patches * 8u);
    std::printf("terrain maps ok\n");
  });
}
