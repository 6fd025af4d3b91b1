// shim_terrain_brush <dir>: runs one brush stroke through ox::amd::apply_terrain_brush of RendererInstance.hpp: trace, apply and the three
// regional passes, as RendererInstance::apply_terrain_brush does with painting set.  Reads <dir>/params.bin ({oxc_terrain_brush_params,
// oxc_terrain_generate, oxc_terrain_derive}) and the seven images <dir>/<name>.bin, and writes the images and the two records as
// <dir>/<name>.out.  tests/test_gpu_terrain_brush_shim.py compares them with the Python path's bytes.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "RendererInstance.hpp"

using namespace ox::amd;

struct Params {
  GPU::TerrainBrushParams brush;
  GPU::TerrainGenerate generate;
  GPU::TerrainDerive derive;
};

static std::vector<char> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return {std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()};
}

static Buffer device_buffer(size_t bytes, const std::string* path = nullptr) {
  void* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess || hipMemset(dev, 0, bytes) != hipSuccess) throw std::runtime_error("hipMalloc failed");
  if (path) {
    const std::vector<char> host = read_file(*path);
    if (host.size() != bytes || hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("upload failed: " + *path);
  }
  return Buffer{dev, bytes};
}

static void write_out(const std::string& path, const void* dptr, size_t bytes) {
  std::vector<char> host(bytes);
  if (hipMemcpy(host.data(), dptr, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("read back failed");
  std::ofstream(path, std::ios::binary).write(host.data(), (std::streamsize)host.size());
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: shim_terrain_brush <dir>\n");
    return 2;
  }
  try {
    const std::string dir = argv[1];
    const std::vector<char> raw = read_file(dir + "/params.bin");
    if (raw.size() != sizeof(Params)) throw std::runtime_error("params.bin has the wrong size");
    const Params& p = *reinterpret_cast<const Params*>(raw.data());
    const size_t texels = (size_t)p.brush.resolution[0] * p.brush.resolution[1], patches = (size_t)p.brush.patch_count[0] * p.brush.patch_count[1];
    RendererInstance self(0);
    const struct {
      const char* name;
      size_t bytes;
    } images[] = {{"heightmap", texels * 2u},   {"ridgemap", texels * 2u},   {"normalmap", texels * 4u},   {"splatmap", texels * 4u},
                  {"height_edit", texels * 4u}, {"splat_edit", texels * 4u}, {"patch_minmax", patches * 8u}};
    Buffer b[7];
    for (int k = 0; k < 7; k++) {
      const std::string path = dir + "/" + images[k].name + ".bin";
      b[k] = device_buffer(images[k].bytes, &path);
    }
    TerrainBrushContext context = {};
    context.maps.renderer = &self;
    context.maps.heightmap = b[0], context.maps.ridgemap = b[1], context.maps.normalmap = b[2], context.maps.splatmap = b[3];
    context.maps.height_edit = b[4], context.maps.splat_edit = b[5];
    context.maps.patch_minmax.dptr = b[6].dptr;
    context.maps.patch_minmax.width = p.brush.patch_count[0], context.maps.patch_minmax.height = p.brush.patch_count[1], context.maps.patch_minmax.levels = 1;
    context.maps.region = device_buffer(sizeof(GPU::TerrainRegion));
    context.hit_buffer = device_buffer(sizeof(GPU::TerrainBrushHit));
    context.params = p.brush;
    context.painting = true;
    context.generate_settings = p.generate;
    context.derive_settings = p.derive;
    apply_terrain_brush(context);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the passes failed");
    for (int k = 0; k < 7; k++) write_out(dir + "/" + images[k].name + ".out", b[k].dptr, images[k].bytes);
    write_out(dir + "/hit.out", context.hit_buffer.dptr, 16);
    write_out(dir + "/region.out", context.maps.region.dptr, 16);
    std::printf("terrain brush ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
