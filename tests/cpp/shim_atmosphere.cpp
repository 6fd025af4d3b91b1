// shim_atmosphere <dir>: takes the atmosphere branch through ox::amd::RendererInstance::apply_pbr.  Reads <dir>/params.bin ({u32 width, height,
// cube_size, pad; float inv_projection_view[16], camera[3], sun_dir[3], sun_intensity; oxc_atmosphere}) and one raw file per image, sets
// HasAtmosphere in gpu_scene_flags, calls apply_pbr and writes <dir>/final.bin.  tests/test_gpu_pbr_atmosphere_shim.py compares it with the checker.
#include <filesystem>

#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  uint32_t width, height, cube_size, pad;
  float inv_projection_view[16], camera[3], sun_dir[3], sun_intensity;
  oxc_atmosphere atmosphere;
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_atmosphere", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    RendererInstance self(0);
    self.gpu_scene_flags = OXC_SCENE_HAS_ATMOSPHERE | OXC_SCENE_HAS_DIRECTIONAL_LIGHT | OXC_SCENE_HAS_CONTACT_SHADOWS;
    self.atmosphere = p.atmosphere;
    for (int i = 0; i < 16; i++) self.camera.inv_projection_view[i] = p.inv_projection_view[i];
    for (int i = 0; i < 3; i++) self.camera.position[i] = p.camera[i], self.directional_light.direction[i] = p.sun_dir[i];
    self.directional_light.intensity = p.sun_intensity;
    // the sizes of the LUTs and images are the test's: each buffer is as large as its file
    const auto upload = [&](const char* name) {
      const std::string path = dir + "/" + name + ".bin";
      return device_buffer(std::filesystem::file_size(path), no_fill, path);
    };
    self.prepared_frame.lights_buffer = upload("lights");
    const auto image = [&](const char* name) {
      ImageAttachment a = {};
      a.dptr = upload(name).dptr;
      a.width = p.width, a.height = p.height, a.levels = 1;
      return a;
    };
    PBRContext context = {};
    context.sky_transmittance_lut_attachment = upload("transmittance");
    context.sky_aerial_perspective_lut_attachment = upload("aerial");
    context.sky_view_lut_attachment = upload("sky_view");
    context.sky_cubemap_attachment = upload("cube");
    context.depth_attachment = image("depth");
    context.albedo_attachment = upload("albedo");
    context.normal_attachment = upload("normal");
    context.emissive_attachment = upload("emissive");
    context.metallic_roughness_occlusion_attachment = upload("mro");
    context.ambient_occlusion_attachment = upload("ao");
    context.contact_shadows_attachment = image("contact");
    context.resolved_shadows_attachment = image("resolved");
    const Buffer out = device_buffer((size_t)p.width * p.height * 4u, no_fill);
    write_out(dir + "/final.bin", self.apply_pbr(context, out));
    // the same context without the flag still takes the no-atmosphere branch
    self.gpu_scene_flags &= ~OXC_SCENE_HAS_ATMOSPHERE;
    self.apply_pbr(context, out);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the no-atmosphere branch failed");
    std::printf("atmosphere branch ok\n");
  });
}
