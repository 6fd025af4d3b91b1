// oxcull_vsm.hip -- VSM page update (gfx950): the page-management passes of Oxylus/src/Render/Passes/Shadowmaps.cpp:143-421.
//
// Four launches instead of the reference's eight passes (rules and orders: include/oxcull.h):
//   k_vsm_reset_invalidate  one 16 x 16 tile of one layer per block: sun_moved clear, reset, invalidation (rmvsm_reset_page_visibility,
//                           rmvsm_invalidate_pages), and the zeroing of the per-page mark map;
//   k_vsm_mark              the per-pixel pass (rmvsm_mark_visible_pages): 4 pixels per lane from one 16-byte load, pages deduplicated
//                           inside the wave (the reference's scalarization loop), one byte store of 1 per distinct page;
//   k_vsm_resolve           ONE block over the whole table: Visible bits, free invisible pages, occupancy, free list, allocation and
//                           the dirty list by block-wide prefix sums -- ascending orders, no global atomics
//                           (rmvsm_free_invisible_pages, _build_free_page_list, _allocate_pages, _mark_dirty_pages);
//   k_vsm_clear             the dirty physical pages set to 1.0 with 16-byte stores (rmvsm_clear_dirty_pages), optional.
// The HPB between resolve and clear is oxcull_hpb.hip's k_generate_hpb (the bytes of oxc_generate_hpb).
//
// Why the per-pixel pass only has to MARK: reset clears every Visible bit before it, so "became visible this frame"
// (mark_visible_pages.slang:70) is "Visible after marking", and everything the reference derives from that first visit
// (occupancy, requests) is a function of the marked set and the table, which the resolve pass reads once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr uint32_t kVsmTile = 16;            // reset / invalidate: 16 x 16 pages per block
constexpr uint32_t kVsmResolveThreads = 1024;
constexpr uint32_t kVsmMarkRows = 4;         // pixel pass: one row segment of 256 pixels per wave, 4 rows per block
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kVisible = 1u, kDirty = 2u, kBacked = 4u, kInvalidated = 8u;
}  // namespace

// ---- pass 1-3: sun_moved clear, reset page visibility, invalidate pages ----------------------------------------------
// Each block recomputes the page rectangles of every (dirty mesh instance, previous / current transform) pair for its layer
// (rmvsm_invalidate_pages.slang:21-60) and tests its own 256 entries against them: no two threads write one entry.
__global__ __launch_bounds__(256) void k_vsm_reset_invalidate(VsmArgs a) {
  __shared__ int4 rects[256];
  const uint32_t layer = blockIdx.y;
  const uint32_t tiles_x = (a.n + kVsmTile - 1) / kVsmTile;
  const uint32_t wx = (blockIdx.x % tiles_x) * kVsmTile + threadIdx.x % kVsmTile;
  const uint32_t wy = (blockIdx.x / tiles_x) * kVsmTile + threadIdx.x / kVsmTile;
  const bool mine = wx < a.n && wy < a.n;
  const size_t e = ((size_t)layer * a.n + wy) * a.n + wx;
  uint32_t v = 0;
  if (mine) {
    v = a.sun_moved ? 0u : a.page_table[e];
    v &= ~(kVisible | kDirty | kInvalidated);
    a.mark[e] = 0;
  }
  if (a.invalidate) {
    const float* cm = a.clipmaps + (size_t)layer * 19;
    float pv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) pv[k] = cm[k];
    const int off_x = __builtin_bit_cast(int, cm[16]), off_y = __builtin_bit_cast(int, cm[17]);
    const float z_near = cm[18];
    const int n = (int)a.n;
    // the virtual coords of this thread's wrapped page: wrapped = floor_mod(virt + offset, n) is a bijection of [0, n)
    const int vx = floor_mod_i((int)wx - floor_mod_i(off_x, n), n), vy = floor_mod_i((int)wy - floor_mod_i(off_y, n), n);
    const uint32_t pairs = a.dirty_count * 2u;
    for (uint32_t base = 0; base < pairs; base += 256) {
      __syncthreads();  // (the previous batch's rectangles are read)
      int4 r = make_int4(1, 1, 0, 0);  // empty
      const uint32_t p = base + threadIdx.x;
      if (p < pairs) {
        const uint32_t id = a.dirty_ids[p >> 1];
        if (id < a.mesh_instance_count) {
          const GpuMeshInstance mi = a.mesh_instances[id];
          const bool prev = (p & 1u) == 0u;  // previous transform first, as the shader does
          if (mi.mesh_index < a.mesh_count && mi.transform_index < (prev ? a.transform_previous_count : a.transform_count)) {
            const float* wsrc = (prev ? a.transforms_previous : a.transforms) + (size_t)mi.transform_index * 16;
            float w[16], mvp[16];
#pragma unroll
            for (int k = 0; k < 16; k++) w[k] = wsrc[k];
            mul_mat4(pv, w, mvp);
            const GpuMesh& m = a.meshes[mi.mesh_index];
            float sa[6];
            if (project_aabb(mvp, z_near, m.aabb_center[0], m.aabb_center[1], m.aabb_center[2], m.aabb_extent[0], m.aabb_extent[1],
                             m.aabb_extent[2], sa)) {
              const float u0 = saturate_f(sa[0]), v0 = saturate_f(sa[1]), u1 = saturate_f(sa[3]), v1 = saturate_f(sa[4]);
              if (!(u0 >= u1) && !(v0 >= v1)) {
                const float fn = (float)a.n;
                r.x = min(max((int)floorf(u0 * fn), 0), n - 1);
                r.y = min(max((int)floorf(v0 * fn), 0), n - 1);
                r.z = min(max((int)ceilf(u1 * fn) - 1, 0), n - 1);
                r.w = min(max((int)ceilf(v1 * fn) - 1, 0), n - 1);
              }
            }
          }
        }
      }
      rects[threadIdx.x] = r;
      __syncthreads();
      if (mine && (v & kBacked)) {
        const uint32_t cnt = min(256u, pairs - base);
        for (uint32_t k = 0; k < cnt; k++) {
          const int4 q = rects[k];
          if (vx >= q.x && vx <= q.z && vy >= q.y && vy <= q.w) {
            v = kInvalidated;  // reset() then set_invalidated(true): the address goes too
            break;
          }
        }
      }
    }
  }
  if (mine) a.page_table[e] = v;
}

// ---- pass 4: mark visible pages ---------------------------------------------------------------------------------------
// The page (linear entry index) pixel (px, py) with depth d marks, or kNone.
OXC_DEV uint32_t pixel_page(const VsmArgs& a, const float* cms, uint32_t px, uint32_t py, float d) {
  if (d == 0.0f) return kNone;  // mark_visible_pages.slang:39
  const float u = ((float)px + 0.5f) / (float)a.depth_w, v = ((float)py + 0.5f) / (float)a.depth_h;
  float cx, cy, cz, lx, ly, lz, rx, ry, rz;
  unproject(a.inv_pv, u, v, d, cx, cy, cz);
  unproject(a.inv_pv, u + -a.off_x, v + a.off_y, d, lx, ly, lz);  // left  = uv + (-o.x, o.y)
  unproject(a.inv_pv, u + a.off_x, v + a.off_y, d, rx, ry, rz);   // right = uv + ( o.x, o.y)
  const float dx = lx - rx, dy = ly - ry, dz = lz - rz;
  const float dist = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
  const float r = dist / a.texel_len;
  uint32_t idx = a.lvl_always;  // (the loop of oxcull_vsm_resolve.hip's kernel: the two must select the same clipmap)
  for (uint32_t k = a.lvl_always; k + 1 < a.layers; k++) idx += (r > a.lvl_thr[k]) ? 1u : 0u;  // NaN: never
  const float* c = cms + idx * 19;
  const float hx = ((OXC_M(c, 0, 0) * cx + OXC_M(c, 0, 1) * cy) + OXC_M(c, 0, 2) * cz) + OXC_M(c, 0, 3);
  const float hy = ((OXC_M(c, 1, 0) * cx + OXC_M(c, 1, 1) * cy) + OXC_M(c, 1, 2) * cz) + OXC_M(c, 1, 3);
  const float hw = ((OXC_M(c, 3, 0) * cx + OXC_M(c, 3, 1) * cy) + OXC_M(c, 3, 2) * cz) + OXC_M(c, 3, 3);
  const float su = (hx / hw + 1.0f) * 0.5f, sv = (hy / hw + 1.0f) * 0.5f;
  if (!(su >= 0.0f && su <= 1.0f && sv >= 0.0f && sv <= 1.0f)) return kNone;  // outside, or NaN
  uint32_t wx, wy;
  if (!wrapped_page(c, su, sv, (float)a.n, (int)a.n, wx, wy)) return kNone;
  return (idx * a.n + wy) * a.n + wx;
}

__global__ __launch_bounds__(256) void k_vsm_mark(VsmArgs a) {
  __shared__ float cms[16 * 19];
  for (uint32_t i = threadIdx.x; i < a.layers * 19; i += blockDim.x) cms[i] = a.clipmaps[i];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t py = blockIdx.y * kVsmMarkRows + (threadIdx.x >> 6);
  const uint32_t px0 = blockIdx.x * 256u + lane * 4u;
  if (py >= a.depth_h) return;  // (whole wave)
  uint32_t pg[4] = {kNone, kNone, kNone, kNone};
  if (px0 < a.depth_w) {
    const float* row = a.depth + (size_t)py * a.depth_w;
    float d[4];
    if (a.depth_vec4) {
      const float4 q = *reinterpret_cast<const float4*>(row + px0);
      d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) d[j] = px0 + j < a.depth_w ? row[px0 + j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (px0 + j < a.depth_w) pg[j] = pixel_page(a, cms, px0 + j, py, d[j]);
  }
  // Scalarization loop: the wave takes the first pending page of its first pending lane, every lane drops it from its four
  // slots, that lane stores.  Marking is idempotent, so the deduplication changes no result.
  for (;;) {
    const uint32_t cur = pg[0] != kNone ? pg[0] : pg[1] != kNone ? pg[1] : pg[2] != kNone ? pg[2] : pg[3];
    const uint64_t m = __builtin_amdgcn_ballot_w64(cur != kNone);
    if (m == 0) break;
    const int first = __builtin_ctzll(m);
    const uint32_t u = readlane_u(cur, first);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (pg[j] == u) pg[j] = kNone;
    if ((int)lane == first) a.mark[u] = 1;
  }
}

// ---- pass 5-7 and 9: free invisible pages, free list, allocation, dirty list -------------------------------------------
namespace {
// Exclusive rank of `pred` among the block's threads in thread order; `total` = the block's count.  Every thread must call it.
OXC_DEV uint32_t block_rank(bool pred, uint32_t* wsum, uint32_t& total) {
  const uint64_t b = __builtin_amdgcn_ballot_w64(pred);
  const uint32_t lane_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
  const uint32_t wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) wsum[wid] = (uint32_t)__builtin_popcountll(b);
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < kVsmResolveThreads / 64; w++) {
    const uint32_t c = wsum[w];
    before += w < wid ? c : 0u;
    all += c;
  }
  __syncthreads();  // (wsum is written again by the next call)
  total = all;
  return before + lane_rank;
}
}  // namespace

__global__ __launch_bounds__(kVsmResolveThreads) void k_vsm_resolve(VsmArgs a) {
  __shared__ uint32_t occ[65536 / 32];  // physical page occupancy (page_occupancy), one bit per page
  __shared__ uint32_t wsum[kVsmResolveThreads / 64];
  __shared__ uint32_t layer_dirty[16];
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < (a.phys_count + 31) / 32; i += kVsmResolveThreads) occ[i] = 0;
  if (t < 16) layer_dirty[t] = 0;
  __syncthreads();
  const uint32_t total = a.layers * a.n * a.n;
  // Visible bits, free invisible pages (Backed bit only), occupancy of the pages that stay backed.  Each thread keeps the entries
  // e = t + k * 1024 for itself: the allocation step below reads back only its own stores.
  for (uint32_t e = t; e < total; e += kVsmResolveThreads) {
    const uint32_t v0 = a.page_table[e];
    uint32_t v = v0;
    if (a.mark[e]) {
      v |= kVisible;
      const uint32_t addr = v >> 16;
      if ((v & kBacked) && addr < a.phys_count) atomicOr(&occ[addr >> 5], 1u << (addr & 31u));
    } else {
      v &= ~kBacked;
    }
    if (v != v0) a.page_table[e] = v;
  }
  __syncthreads();
  // free page list, ascending physical index
  uint32_t free_count = 0;
  for (uint32_t base = 0; base < a.phys_count; base += kVsmResolveThreads) {
    const uint32_t p = base + t;
    const bool is_free = p < a.phys_count && !((occ[p >> 5] >> (p & 31u)) & 1u);
    uint32_t cnt;
    const uint32_t r = block_rank(is_free, wsum, cnt);
    if (is_free) a.free_list[free_count + r] = p;
    free_count += cnt;
  }
  __syncthreads();  // (the free list is read by other threads of the block below)
  // allocation: request i (ascending (layer, y, x)) takes free_list[i]; the pages allocated here are the dirty list, in the same order
  uint32_t requests = 0;
  for (uint32_t base = 0; base < total; base += kVsmResolveThreads) {
    const uint32_t e = base + t;
    uint32_t v = e < total ? a.page_table[e] : 0u;
    const bool req = e < total && (v & (kVisible | kBacked)) == kVisible;
    uint32_t cnt;
    const uint32_t r = requests + block_rank(req, wsum, cnt);
    if (req && r < free_count) {
      const uint32_t addr = a.free_list[r];
      v = (v & 0xFFFFu) | (addr << 16) | kDirty | kBacked;  // set_physical_address, set_dirty, set_backed
      a.page_table[e] = v;
      a.dirty_coords[2 * r] = addr % a.phys_side;
      a.dirty_coords[2 * r + 1] = addr / a.phys_side;
      layer_dirty[e / (a.n * a.n)] = 1u;
    }
    requests += cnt;
  }
  __syncthreads();
  const uint32_t dirty = min(requests, free_count);
  if (t < a.layers) a.dirty_flags[t] = layer_dirty[t];
  if (t == 0) {
    a.counters[0] = requests;  // active_request_count
    a.counters[1] = dirty;     // dirty_physical_page_count
    a.counters[2] = free_count;
    a.counters[3] = requests;  // alloc_cursor: every request pops a slot, failed or not
    a.counters[4] = requests - dirty;
    a.counters[5] = a.counters[6] = a.counters[7] = 0;
    a.clear_cmd[0] = a.page_size / 16u;
    a.clear_cmd[1] = a.page_size / 16u;
    a.clear_cmd[2] = dirty;
  }
}

// ---- pass 10: clear dirty pages ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vsm_clear(VsmArgs a) {
  const uint32_t count = a.counters[1];
  const uint32_t q = a.page_size / 4u;  // float4 per page row
  const float4 one = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
  for (uint32_t p = blockIdx.x; p < count; p += gridDim.x) {
    const uint32_t cx = a.dirty_coords[2 * p], cy = a.dirty_coords[2 * p + 1];
    float* origin = a.physical + ((size_t)cy * a.page_size) * a.physical_size + (size_t)cx * a.page_size;
    for (uint32_t i = threadIdx.x; i < a.page_size * q; i += blockDim.x) {
      const uint32_t y = i / q, x4 = i % q;
      *reinterpret_cast<float4*>(origin + (size_t)y * a.physical_size + x4 * 4u) = one;
    }
  }
}

void launch_vsm_update(const VsmArgs& a, uint32_t num_cus, uint8_t* hpb, uint32_t hpb_levels, const uint64_t* hpb_level_offset, hipStream_t s) {
  const uint32_t tiles = (a.n + kVsmTile - 1) / kVsmTile;
  hipLaunchKernelGGL(k_vsm_reset_invalidate, dim3(tiles * tiles, a.layers), dim3(256), 0, s, a);
  if (a.depth_w && a.depth_h)
    hipLaunchKernelGGL(k_vsm_mark, dim3((a.depth_w + 255) / 256, (a.depth_h + kVsmMarkRows - 1) / kVsmMarkRows), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_vsm_resolve, dim3(1), dim3(kVsmResolveThreads), 0, s, a);
  if (hpb) launch_generate_hpb(a.page_table, hpb, a.n, a.n, a.layers, hpb_levels, hpb_level_offset, s);
  if (a.physical) {
    const uint32_t grid = std::min(a.phys_count, num_cus * 4u);
    hipLaunchKernelGGL(k_vsm_clear, dim3(grid), dim3(256), 0, s, a);
  }
}

}  // namespace oxc
