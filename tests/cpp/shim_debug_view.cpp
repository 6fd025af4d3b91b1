// shim_debug_view <dir>: runs the fourteen main debug views through RendererInstance::apply_debug_view of RendererInstance.hpp.  Reads
// <dir>/params.bin (Params below), the eight images and the three record buffers as <dir>/<name>.bin, and writes the debug attachment of
// view k as <dir>/view<k>.out.  tests/test_gpu_debug_view_shim.py compares them with the golden fixture's bytes.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "RendererInstance.hpp"

using namespace ox::amd;

struct Params {
  uint32_t width, height;
  uint32_t meshlet_instances, mesh_instances, meshes;  // record counts
  float heatmap_scale;
};

static std::vector<char> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return {std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()};
}

static Buffer device_buffer(size_t bytes, const std::string& path) {
  void* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess) throw std::runtime_error("hipMalloc failed");
  const std::vector<char> host = read_file(path);
  if (host.size() != bytes || hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("upload failed: " + path);
  return Buffer{dev, bytes};
}

static void write_out(const std::string& path, const Buffer& b) {
  std::vector<char> host(b.bytes);
  if (hipMemcpy(host.data(), b.dptr, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("read back failed");
  std::ofstream(path, std::ios::binary).write(host.data(), (std::streamsize)host.size());
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: shim_debug_view <dir>\n");
    return 2;
  }
  try {
    const std::string dir = argv[1];
    const std::vector<char> raw = read_file(dir + "/params.bin");
    if (raw.size() != sizeof(Params)) throw std::runtime_error("params.bin has the wrong size");
    const Params& p = *reinterpret_cast<const Params*>(raw.data());
    const size_t pixels = (size_t)p.width * p.height;
    RendererInstance self(0);
    const auto load = [&](const char* name, size_t bytes) { return device_buffer(bytes, dir + "/" + name + ".bin"); };
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
    void* out = nullptr;
    if (hipMalloc(&out, pixels * 8u) != hipSuccess) throw std::runtime_error("hipMalloc failed");
    context.debug_attachment = Buffer{out, pixels * 8u};
    for (uint32_t view = OXC_DEBUG_VIEW_TRIANGLES; view <= OXC_DEBUG_VIEW_GEOMETRIC_NORMAL; view++) {
      if (hipMemset(out, 0xEE, pixels * 8u) != hipSuccess) throw std::runtime_error("hipMemset failed");
      context.debug_view = view;
      const Buffer written = self.apply_debug_view(context, Extent3D{p.width, p.height, 1});
      if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the pass failed");
      write_out(dir + "/view" + std::to_string(view) + ".out", written);
    }
    std::printf("debug views ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
