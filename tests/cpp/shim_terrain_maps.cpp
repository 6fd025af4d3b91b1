// shim_terrain_maps <dir>: runs the three terrain passes through the free functions of RendererInstance.hpp, one after the other, as
// Terrain::bake does.  Reads <dir>/params.bin ({oxc_terrain_generate, oxc_terrain_derive, u32 patch_count[2]}; the resolution is the
// settings') and <dir>/height_edit.bin, <dir>/splat_edit.bin, and writes the five images as <dir>/<name>.out.
// tests/test_gpu_terrain_maps_shim.py compares them with the checker.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "RendererInstance.hpp"

using namespace ox::amd;

struct Params {
  GPU::TerrainGenerate generate;
  GPU::TerrainDerive derive;
  uint32_t patch_count[2];
};

static std::vector<char> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return {std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()};
}

static Buffer device_buffer(size_t bytes, const std::vector<char>* host = nullptr) {
  void* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess || hipMemset(dev, 0, bytes) != hipSuccess) throw std::runtime_error("hipMalloc failed");
  if (host && (host->size() != bytes || hipMemcpy(dev, host->data(), bytes, hipMemcpyHostToDevice) != hipSuccess)) throw std::runtime_error("upload failed");
  return Buffer{dev, bytes};
}

static void write_out(const std::string& path, const void* dptr, size_t bytes) {
  std::vector<char> host(bytes);
  if (hipMemcpy(host.data(), dptr, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("read back failed");
  std::ofstream(path, std::ios::binary).write(host.data(), (std::streamsize)host.size());
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: shim_terrain_maps <dir>\n");
    return 2;
  }
  try {
    const std::string dir = argv[1];
    const std::vector<char> raw = read_file(dir + "/params.bin");
    if (raw.size() != sizeof(Params)) throw std::runtime_error("params.bin has the wrong size");
    const Params& p = *reinterpret_cast<const Params*>(raw.data());
    const uvec2 resolution = {p.generate.resolution[0], p.generate.resolution[1]}, patch_count = {p.patch_count[0], p.patch_count[1]};
    const size_t texels = (size_t)resolution.x * resolution.y, patches = (size_t)patch_count.x * patch_count.y;
    RendererInstance self(0);
    const std::vector<char> height_edit = read_file(dir + "/height_edit.bin"), splat_edit = read_file(dir + "/splat_edit.bin");
    TerrainMaps maps = {};
    maps.renderer = &self;
    maps.heightmap = device_buffer(texels * 2u);
    maps.ridgemap = device_buffer(texels * 2u);
    maps.normalmap = device_buffer(texels * 4u);
    maps.splatmap = device_buffer(texels * 4u);
    maps.height_edit = device_buffer(texels * 4u, &height_edit);
    maps.splat_edit = device_buffer(texels * 4u, &splat_edit);
    maps.patch_minmax.dptr = device_buffer(patches * 8u).dptr;
    maps.patch_minmax.width = patch_count.x, maps.patch_minmax.height = patch_count.y, maps.patch_minmax.levels = 1;
    GPU::TerrainMinMax minmax_settings = {};
    minmax_settings.resolution[0] = resolution.x, minmax_settings.resolution[1] = resolution.y;
    minmax_settings.patch_count[0] = patch_count.x, minmax_settings.patch_count[1] = patch_count.y;
    terrain_generate_pass(maps, p.generate, resolution);
    terrain_derive_pass(maps, p.derive, resolution);
    terrain_minmax_pass(maps, minmax_settings, patch_count);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the passes failed");
    write_out(dir + "/heightmap.out", maps.heightmap.dptr, texels * 2u);
    write_out(dir + "/ridgemap.out", maps.ridgemap.dptr, texels * 2u);
    write_out(dir + "/normalmap.out", maps.normalmap.dptr, texels * 4u);
    write_out(dir + "/splatmap.out", maps.splatmap.dptr, texels * 4u);
    write_out(dir + "/patch_minmax.out", maps.patch_minmax.dptr, patches * 8u);
    std::printf("terrain maps ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
