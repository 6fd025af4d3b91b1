// shim_sprites <dir>: runs the 2D pass through RendererInstance::draw_sprites and RendererInstance::pick_sprite of RendererInstance.hpp.
// Reads <dir>/params.bin (Params below) and the inputs as <dir>/<name>.bin; for source format f and stage set s it writes the depth, the
// visbuffer and the colour image as <dir>/<image>_format<f>_stages<s>.out, and the picked word as <dir>/pick.out.
// tests/test_gpu_sprites_shim.py compares them with the golden fixture's bytes.
#include "shim_io.hpp"

using namespace ox::amd;
using namespace shim_io;

struct Params {
  uint32_t width, height;
  uint32_t sprites, materials, transforms;  // record counts
  uint32_t pick_x, pick_y;
};

int main(int argc, char** argv) {
  return run(argc, argv, "shim_sprites", [](const std::string& dir) {
    const Params p = read_params<Params>(dir);
    const size_t pixels = (size_t)p.width * p.height;
    const Extent3D extent = {p.width, p.height, 1};
    RendererInstance self(0);
    const auto load = [&](const std::string& name, size_t bytes) { return device_buffer(bytes, 0xEE, dir + "/" + name + ".bin"); };
    self.prepared_frame.transforms_world_buffer = load("transforms", (size_t)p.transforms * 64u);
    self.prepared_frame.materials_buffer = load("materials", (size_t)p.materials * 56u);

    SpriteContext context = {};
    context.sprites_buffer = load("sprites", (size_t)p.sprites * 12u);
    context.batch_count = p.sprites;
    const std::vector<char> pv = read_file(dir + "/pv.bin");
    if (pv.size() != 64u) throw std::runtime_error("pv.bin has the wrong size");
    for (int i = 0; i < 16; i++) context.projection_view[i] = reinterpret_cast<const float*>(pv.data())[i];
    context.visbuffer_attachment_2d = device_buffer(pixels * 4u, 0xEE);
    for (uint32_t format = 0; format < 2; format++)
      for (uint32_t stages = 1; stages <= 3; stages++) {
        const std::string tag = "_format" + std::to_string(format) + "_stages" + std::to_string(stages) + ".out";
        const Buffer depth = load("depth", pixels * 4u);
        ImageAttachment depth_attachment = {};
        depth_attachment.dptr = depth.dptr;
        depth_attachment.width = p.width, depth_attachment.height = p.height, depth_attachment.levels = 1;
        const Buffer color = load("color_format" + std::to_string(format), pixels * (format ? 8u : 4u));
        self.draw_sprites(context, stages, extent, depth_attachment, color, format);
        write_out(dir + "/depth" + tag, depth);
        if (stages & OXC_SPRITES_VIS) write_out(dir + "/vis" + tag, context.visbuffer_attachment_2d);
        if (stages & OXC_SPRITES_COLOR) write_out(dir + "/color" + tag, color);
      }
    SpritePickingContext picking = {};
    picking.picking_texel[0] = p.pick_x, picking.picking_texel[1] = p.pick_y;
    picking.visbuffer_attachment_2d = context.visbuffer_attachment_2d;  // the last call ran both stages
    picking.transform_id = device_buffer(4u, 0xEE);
    write_out(dir + "/pick.out", self.pick_sprite(picking, extent));
    std::printf("sprites ok\n");
  });
}
