// shim_textured_decode <dir>: runs one textured visbuffer decode through RendererInstance::decode_visbuffer(context, images, samplers) of
// RendererInstance.hpp.  Reads <dir>/params.bin (Params below) and the scene, the frame and the two tables, <dir>/<name>.bin.  A pointer
// field of the Mesh, MeshLOD and image records holds 1 + the byte offset into the stream it points into (0: null); the program uploads the
// streams and writes the device addresses in.  Writes the four attachments as <dir>/<name>.out.  tests/test_gpu_textured_decode_shim.py
// compares them with the Python path's bytes.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  uint32_t width, height;
  uint32_t meshlet_instances, mesh_instances, meshes, materials, images, samplers;  // record counts
  float projection_view[16];
  float camera_position[3];
  uint32_t pad;
};

namespace {
Buffer upload(const std::vector<char>& host) {
  void* dev = nullptr;
  const size_t bytes = host.size() ? host.size() : 4;
  if (hipMalloc(&dev, bytes) != hipSuccess || hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("upload failed");
  return Buffer{dev, host.size()};
}
// field `word` (in u64 units) of every `stride`-byte record: 1 + offset -> address inside `stream`
void relocate(std::vector<char>& records, size_t stride, size_t word, const Buffer& stream) {
  for (size_t at = 0; at + stride <= records.size(); at += stride) {
    uint64_t v;
    std::memcpy(&v, records.data() + at + word * 8, 8);
    v = v ? reinterpret_cast<uint64_t>(stream.dptr) + (v - 1) : 0;
    std::memcpy(records.data() + at + word * 8, &v, 8);
  }
}
}  // namespace

int main(int argc, char** argv) {
  return run(argc, argv, "shim_textured_decode", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const size_t pixels = (size_t)p.width * p.height;
    RendererInstance self(0);
    const auto file = [&](const char* name) { return read_file(dir + "/" + name + ".bin"); };
    const auto load = [&](const char* name, size_t bytes) { return device_buffer(bytes, no_fill, dir + "/" + name + ".bin"); };
    const Buffer positions = upload(file("positions")), normals = upload(file("normals")), texcoords = upload(file("texcoords"));
    const Buffer meshlets = upload(file("meshlets")), micro = upload(file("micro")), vidx = upload(file("vidx")), texels = upload(file("texels"));
    std::vector<char> lods = file("lods"), meshes = file("meshes"), images = file("images");
    relocate(lods, 64, 1, meshlets), relocate(lods, 64, 3, micro), relocate(lods, 64, 4, vidx);  // GPU::MeshLOD
    const Buffer lods_buffer = upload(lods);
    relocate(meshes, 64, 0, positions), relocate(meshes, 64, 1, normals), relocate(meshes, 64, 2, texcoords), relocate(meshes, 64, 4, lods_buffer);  // GPU::Mesh
    relocate(images, sizeof(oxc_material_image), 0, texels);
    if (meshes.size() != (size_t)p.meshes * 64u || images.size() != (size_t)p.images * sizeof(oxc_material_image)) throw std::runtime_error("record counts differ from params.bin");

    self.prepared_frame.mesh_instance_count = p.mesh_instances;
    self.prepared_frame.max_meshlet_instance_count = p.meshlet_instances;
    self.prepared_frame.meshes_buffer = upload(meshes);
    self.prepared_frame.meshlet_instances_buffer = load("meshlet_instances", (size_t)p.meshlet_instances * 8u);
    self.prepared_frame.mesh_instances_buffer = load("mesh_instances", (size_t)p.mesh_instances * 20u);
    self.prepared_frame.transforms_world_buffer = load("transforms", (size_t)p.mesh_instances * 64u);
    self.prepared_frame.materials_buffer = load("materials", (size_t)p.materials * 56u);

    MainGeometryContext context = {};
    for (int k = 0; k < 16; k++) context.cull_camera.projection_view[k] = p.projection_view[k];
    for (int k = 0; k < 3; k++) context.cull_camera.position[k] = p.camera_position[k];
    const Buffer depth = load("depth", pixels * 4u);
    context.depth_attachment.dptr = depth.dptr;
    context.depth_attachment.width = p.width, context.depth_attachment.height = p.height, context.depth_attachment.levels = 1;
    context.visbuffer_attachment = load("vis", pixels * 4u);
    context.albedo_attachment = device_buffer(pixels * 4u, 0xFB);
    context.normal_attachment = device_buffer(pixels * 8u, 0xFB);
    context.emissive_attachment = device_buffer(pixels * 4u, 0xFB);
    context.metallic_roughness_occlusion_attachment = device_buffer(pixels * 4u, 0xFB);
    self.decode_visbuffer(context, upload(images), load("samplers", (size_t)p.samplers * sizeof(oxc_material_sampler)));
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("the pass failed");
    write_out(dir + "/albedo.out", context.albedo_attachment);
    write_out(dir + "/normal.out", context.normal_attachment);
    write_out(dir + "/emissive.out", context.emissive_attachment);
    write_out(dir + "/mro.out", context.metallic_roughness_occlusion_attachment);
    std::printf("textured decode ok\n");
  });
}
