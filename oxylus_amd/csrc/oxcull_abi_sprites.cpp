// oxcull_abi_sprites.cpp -- the 2D pass of liboxcull.so's C ABI: oxc_pack_sprite and oxc_sort_sprites (the host's RenderQueue2D), oxc_draw_sprites
// (the two sprite passes between oxc_apply_pbr and oxc_apply_fxaa) and oxc_pick_sprite (which sprite lies under a texel).
#include "oxcull_host.hpp"

namespace {
// binary32 -> binary16 bits, round to nearest even, denormals kept, every NaN 0x7E00 (glm::packHalf1x16 stands there in the reference)
uint32_t half_bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  const uint32_t sign = (b >> 16) & 0x8000u, mag = b & 0x7FFFFFFFu;
  if (mag > 0x7F800000u) return 0x7E00u;
  if (mag >= 0x47800000u) return sign | 0x7C00u;  // 65536 and above, Inf included (65520 .. 65536 gets there by the carry below)
  if (mag < 0x33000000u) return sign;  // below 2^-25: rounds to zero (2^-25 itself ties to even, zero)
  const int32_t e = (int32_t)(mag >> 23) - 127;
  const uint32_t m = (mag & 0x7FFFFFu) | 0x800000u;
  const uint32_t shift = e < -14 ? (uint32_t)(13 + (-14 - e)) : 13u;  // a denormal half keeps fewer bits
  const uint32_t kept = m >> shift, rest = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  uint32_t h = e < -14 ? kept : (((uint32_t)(e + 15) << 10) | (kept & 0x3FFu));
  if (rest > half || (rest == half && (h & 1u))) h++;  // a carry out of the mantissa raises the exponent, as it should
  return sign | h;
}

uint32_t half_sort_key(uint32_t bits) { return (bits & 0x8000u) ? (~bits & 0xFFFFu) : (bits | 0x8000u); }

uint64_t sort_key(const oxc_sprite& s) {
  const uint32_t y = (s.flags16_distance16 & OXC_SPRITE_SORT_Y) ? half_sort_key(s.material_id16_ypos16 >> 16) : 0u;
  return ((uint64_t)(s.flags16_distance16 >> 16) << 32) | y;
}
}  // namespace

extern "C" {

oxc_status oxc_pack_sprite(uint32_t render_flags, float position_y, uint32_t transform_id, uint32_t material_id, float distance, oxc_sprite* out) {
  if (!out) return OXC_INVALID_ARG;
  out->material_id16_ypos16 = (material_id & 0xFFFFu) | (half_bits(position_y) << 16);
  out->flags16_distance16 = (render_flags & 0xFFFFu) | (half_bits(distance) << 16);
  out->transform_id = transform_id;
  return OXC_OK;
}

oxc_status oxc_sort_sprites(oxc_sprite* sprites, uint64_t count) {
  if (count == 0u) return OXC_OK;
  if (!sprites) return OXC_INVALID_ARG;
  std::stable_sort(sprites, sprites + count, [](const oxc_sprite& a, const oxc_sprite& b) { return sort_key(a) > sort_key(b); });
  return OXC_OK;
}

oxc_status oxc_draw_sprites(oxc_ctx* ctx, const oxc_prepared_frame* f, const oxc_sprite_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_sprite_context)) return fail(ctx, OXC_INVALID_ARG, "draw_sprites: bad context / struct_size");
  const char* const entry = "draw_sprites";
  const uint32_t stages = c->stages, vis = OXC_SPRITES_VIS, color = OXC_SPRITES_COLOR, both = vis | color;
  if (stages == 0u || (stages & ~both)) return bad_arg(ctx, entry, "stages must be a non-empty set of OXC_SPRITES_VIS and OXC_SPRITES_COLOR");
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (c->width > 16384u || c->height > 16384u) return bad_arg(ctx, entry, "extent beyond 16384");
  if ((stages & color) && c->source_format > 1u) return bad_arg(ctx, entry, "source_format must be 0 (B10G11R11) or 1 (R16G16B16A16 Sfloat)");
  if (c->first_sprite + c->sprite_count < c->first_sprite) return bad_arg(ctx, entry, "first_sprite + sprite_count wraps");
  if (c->sprite_count > kSpriteMaxCount) return bad_arg(ctx, entry, "sprite_count beyond 1048576");
  const oxc_image& dimg = c->depth_attachment;
  if (dimg.width != c->width || dimg.height != c->height) return bad_arg(ctx, entry, "depth_attachment extent differs from (width, height)");
  if (dimg.levels != 1 || dimg.level_offset[0] != 0) return bad_arg(ctx, entry, "depth_attachment must be one R32F level at offset 0");
  if (!f) return bad_arg(ctx, entry, "the frame must not be null");

  const uint64_t pixels = (uint64_t)c->width * c->height;
  const uint32_t texel = (stages & color) && c->source_format == 1u ? 8u : 4u;
  const oxc_buffer& tw = f->transforms_world_buffer;
  const MapBuffer buffers[] = {
      {"sprites_buffer", c->sprites_buffer.dptr, c->sprites_buffer.bytes, ((uint64_t)c->first_sprite + c->sprite_count) * sizeof(oxc_sprite), 4u, both, 0u, false,
       " is smaller than first_sprite + sprite_count records"},
      {"materials_buffer", c->materials_buffer.dptr, c->materials_buffer.bytes, (uint64_t)c->material_count * 56u, 4u, both, 0u, c->material_count == 0u,
       " is smaller than material_count records"},
      {"depth_attachment", dimg.dptr, pixels * 4u, pixels * 4u, 4u, both, both, false},
      {"visbuffer_2d", c->visbuffer_2d.dptr, c->visbuffer_2d.bytes, pixels * 4u, 4u, vis, vis, false},
      {"final_attachment", c->final_attachment.dptr, c->final_attachment.bytes, pixels * texel, texel, color, color, false},
      {"transforms_world_buffer", tw.dptr, tw.bytes, (uint64_t)c->transform_count * 64u, 4u, both, 0u, false, " is smaller than transform_count matrices"},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, stages)) return st;

  OXC_ENTER(ctx, hip_stream, s);
  if (c->sprite_count == 0u) {  // only `clear` acts
    if ((stages & vis) && c->clear) OXC_HIP(ctx, hipMemsetAsync(c->visbuffer_2d.dptr, 0xFF, pixels * 4u, s));
    return OXC_OK;
  }
  SpriteArgs a;
  std::memset(&a, 0, sizeof a);
  a.sprite_count = c->sprite_count, a.material_count = c->material_count, a.transform_count = c->transform_count;
  a.w = c->width, a.h = c->height, a.stages = stages, a.clear = c->clear;
  a.bins_x = cdiv(c->width, kSpriteBin), a.bins_y = cdiv(c->height, kSpriteBin);
  a.list_stride = std::min(c->sprite_count, kSpriteBinCapacity);
  const uint64_t n = c->sprite_count, bins = (uint64_t)a.bins_x * a.bins_y;
  auto layout = [&](Carve& carve) {
    carve.take(a.records, n * sizeof(SpriteRecord));
    carve.take(a.boxes, n * sizeof(uint2));
    carve.take(a.clipped, n * kSpriteMaxTris * sizeof(SpriteTri));
    carve.take(a.bin_counts, bins * 4u);
    carve.take(a.bin_lists, bins * a.list_stride * 4u);
  };
  Carve size;
  layout(size);
  OXC_TRY(grow_scratch(ctx, s, ctx->sprite_scratch, ctx->sprite_scratch_bytes, size.off, (size_t)size.off,
                       "draw_sprites: more sprites or bins than any earlier call (scratch would grow); make one un-captured call first", "hipMalloc(sprite scratch)"));
  Carve bind;
  bind.base = static_cast<char*>(ctx->sprite_scratch);
  layout(bind);
  a.sprites = static_cast<const uint32_t*>(c->sprites_buffer.dptr) + (size_t)c->first_sprite * 3u;
  a.materials = static_cast<const uint32_t*>(c->materials_buffer.dptr);
  a.transforms = static_cast<const float*>(tw.dptr);
  std::memcpy(a.pv, c->projection_view, 64);
  a.depth = static_cast<float*>(dimg.dptr);
  a.vis = (stages & vis) ? static_cast<uint32_t*>(c->visbuffer_2d.dptr) : nullptr;
  a.color = (stages & color) ? c->final_attachment.dptr : nullptr;
  launch_draw_sprites(a, c->source_format, s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

oxc_status oxc_pick_sprite(oxc_ctx* ctx, const oxc_sprite_pick_context* c, void* hip_stream) {
  if (!ctx) return OXC_INVALID_ARG;
  if (!c || c->struct_size != sizeof(oxc_sprite_pick_context)) return fail(ctx, OXC_INVALID_ARG, "pick_sprite: bad context / struct_size");
  const char* const entry = "pick_sprite";
  if (c->width == 0u || c->height == 0u) return bad_arg(ctx, entry, "the extent must not be zero");
  if (c->width > 65536u || c->height > 65536u) return bad_arg(ctx, entry, "extent beyond 65536");
  if (c->x >= c->width || c->y >= c->height) return bad_arg(ctx, entry, "the texel lies outside the image");
  const uint64_t pixels = (uint64_t)c->width * c->height;
  const MapBuffer buffers[] = {
      {"visbuffer_2d", c->visbuffer_2d.dptr, c->visbuffer_2d.bytes, pixels * 4u, 4u, 1u, 0u, false},
      {"transform_id", c->transform_id.dptr, c->transform_id.bytes, 4u, 4u, 1u, 1u, false},
  };
  if (const oxc_status st = check_buffers(ctx, entry, buffers, 1u)) return st;
  OXC_ENTER(ctx, hip_stream, s);
  launch_pick_sprite(static_cast<const uint32_t*>(c->visbuffer_2d.dptr), c->width, c->x, c->y, static_cast<uint32_t*>(c->transform_id.dptr), s);
  OXC_HIP(ctx, hipGetLastError());
  return OXC_OK;
}

}  // extern "C"
