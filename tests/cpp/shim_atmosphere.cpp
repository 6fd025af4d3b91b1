// shim_atmosphere <dir>: takes the atmosphere branch through ox::amd::RendererInstance::apply_pbr.  Reads <dir>/params.bin ({u32 width, height,
// cube_size, pad; float inv_projection_view[16], camera[3], sun_dir[3], sun_intensity; oxc_atmosphere}) and one raw file per image, sets
// HasAtmosphere in gpu_scene_flags, calls apply_pbr and writes <dir>/final.bin.  tests/test_gpu_pbr_atmosphere_shim.py compares it with the checker.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "RendererInstance.hpp"

using namespace ox::amd;

struct Params {
  uint32_t width, height, cube_size, pad;
  float inv_projection_view[16], camera[3], sun_dir[3], sun_intensity;
  oxc_atmosphere atmosphere;
};

static std::vector<char> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return {std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()};
}

static Buffer upload(const std::string& dir, const char* name) {
  const std::vector<char> host = read_file(dir + "/" + name + ".bin");
  void* dev = nullptr;
  if (hipMalloc(&dev, host.size()) != hipSuccess || hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess)
    throw std::runtime_error(std::string("upload failed: ") + name);
  return Buffer{dev, host.size()};
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: shim_atmosphere <dir>\n");
    return 2;
  }
  try {
    const std::string dir = argv[1];
    const std::vector<char> raw = read_file(dir + "/params.bin");
    if (raw.size() != sizeof(Params)) throw std::runtime_error("params.bin has the wrong size");
    const Params& p = *reinterpret_cast<const Params*>(raw.data());
    RendererInstance self(0);
    self.gpu_scene_flags = OXC_SCENE_HAS_ATMOSPHERE | OXC_SCENE_HAS_DIRECTIONAL_LIGHT | OXC_SCENE_HAS_CONTACT_SHADOWS;
    self.atmosphere = p.atmosphere;
    for (int i = 0; i < 16; i++) self.camera.inv_projection_view[i] = p.inv_projection_view[i];
    for (int i = 0; i < 3; i++) self.camera.position[i] = p.camera[i], self.directional_light.direction[i] = p.sun_dir[i];
    self.directional_light.intensity = p.sun_intensity;
    self.prepared_frame.lights_buffer = upload(dir, "lights");
    const auto image = [&](const char* name) {
      ImageAttachment a = {};
      a.dptr = upload(dir, name).dptr;
      a.width = p.width, a.height = p.height, a.levels = 1;
      return a;
    };
    PBRContext context = {};
    context.sky_transmittance_lut_attachment = upload(dir, "transmittance");
    context.sky_aerial_perspective_lut_attachment = upload(dir, "aerial");
    context.sky_view_lut_attachment = upload(dir, "sky_view");
    context.sky_cubemap_attachment = upload(dir, "cube");
    context.depth_attachment = image("depth");
    context.albedo_attachment = upload(dir, "albedo");
    context.normal_attachment = upload(dir, "normal");
    context.emissive_attachment = upload(dir, "emissive");
    context.metallic_roughness_occlusion_attachment = upload(dir, "mro");
    context.ambient_occlusion_attachment = upload(dir, "ao");
    context.contact_shadows_attachment = image("contact");
    context.resolved_shadows_attachment = image("resolved");
    const size_t bytes = (size_t)p.width * p.height * 4u;
    void* out = nullptr;
    if (hipMalloc(&out, bytes) != hipSuccess) throw std::runtime_error("hipMalloc failed");
    const Buffer final_attachment = self.apply_pbr(context, Buffer{out, bytes});
    std::vector<char> host(bytes);
    if (hipMemcpy(host.data(), final_attachment.dptr, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("read back failed");
    std::ofstream(dir + "/final.bin", std::ios::binary).write(host.data(), (std::streamsize)host.size());
    // the same context without the flag still takes the no-atmosphere branch
    self.gpu_scene_flags &= ~OXC_SCENE_HAS_ATMOSPHERE;
    self.apply_pbr(context, Buffer{out, bytes});
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the no-atmosphere branch failed");
    std::printf("atmosphere branch ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
