// oxcull_draw_big.inc -- the bodies of k_draw_big (OXC_BIG_PART 1) and k_draw_big_tiles (OXC_BIG_PART 2) of oxcull_raster.hip, included once
// by each kernel and once more by its counting instantiation.  OXC_BIG_TALLY is the lane's fragment tally handed to the pixel walkers: nullptr
// in the draw's own kernels, which therefore compile to what they were before the counting kernels existed (held by comparing their device
// assembly), a pointer to a local in k_draw_big_count / k_draw_big_tiles_count.  `a` is the kernel's DrawArgs.
#if OXC_BIG_PART == 1
  __shared__ uint32_t s_prefix[kBigSegs + 1];
  __shared__ uint32_t s_wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {  // the segments' fill counts -> exclusive prefix (every block computes the same 256-entry scan)
    static_assert(kBigSegs == 256, "one count per thread");
    const uint32_t c = min(a.big_seg_counts[threadIdx.x * kBigSegStride], a.big_seg_capacity);
    const uint32_t incl = wave_incl_scan(c, lane);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; w++) base += s_wsum[w];
    s_prefix[threadIdx.x + 1] = base + incl;
    if (threadIdx.x == 0) s_prefix[0] = 0;
    __syncthreads();
  }
  const uint32_t total = s_prefix[kBigSegs];
  const uint32_t wave_id = blockIdx.x * 4u + (uint32_t)wave, nwaves = gridDim.x * 4u;
  for (uint32_t i = wave_id; i < total; i += nwaves) {  // wave-uniform
    uint32_t seg = 0;  // the segment task i falls into: the last one whose prefix is <= i
#pragma unroll
    for (uint32_t stp = kBigSegs / 2; stp >= 1u; stp >>= 1)
      if (s_prefix[seg + stp] <= i) seg += stp;
    const uint32_t slot = seg * a.big_seg_capacity + (i - s_prefix[seg]);
    TriRaster r;
    tri_prepare(a.big_list[slot], a.width, a.height, r);
    const uint32_t ntx = (uint32_t)((r.px1 - r.px0 + kBigTile) / kBigTile), nty = (uint32_t)((r.py1 - r.py0 + kBigTile) / kBigTile);
    const uint32_t n = ntx * nty;
    if (n == 1u) {
      raster_rect(a, r, r.px0, r.py0, r.px1, r.py1, lane, OXC_BIG_TALLY);
      continue;
    }
    uint32_t first = 0;
    if (lane == 0) first = atomicAdd(a.tile_count, n);
    first = readlane_u(first, 0);
    for (uint32_t k = (uint32_t)lane; k < n; k += 64u) {
      if (first + k < a.tile_capacity && first + k >= first) a.tile_list[first + k] = make_uint2(slot, k);
    }
    if (first + n > a.tile_capacity || first + n < first) {  // the tile list is full: the tiles that did not fit are walked here (slow, correct)
#pragma clang loop unroll(disable)
      for (uint32_t k = 0; k < n; k++) {
        if (first + k < a.tile_capacity && first + k >= first) continue;
        const int64_t ox = r.px0 + (int64_t)(k % ntx) * kBigTile, oy = r.py0 + (int64_t)(k / ntx) * kBigTile;
        raster_rect64(a, r, ox, oy, min(ox + kBigTile - 1, r.px1), min(oy + kBigTile - 1, r.py1), lane, OXC_BIG_TALLY);
      }
    }
  }
#else
  const uint32_t count = min(*a.tile_count, a.tile_capacity);
  const int lane = threadIdx.x & 63;
  const uint32_t wave_id = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
  for (uint32_t i = wave_id; i < count; i += nwaves) {
    const uint2 item = a.tile_list[i];
    TriRaster r;
    tri_prepare(a.big_list[item.x], a.width, a.height, r);
    const uint32_t ntx = (uint32_t)((r.px1 - r.px0 + kBigTile) / kBigTile);
    const int64_t ox = r.px0 + (int64_t)(item.y % ntx) * kBigTile, oy = r.py0 + (int64_t)(item.y / ntx) * kBigTile;
    raster_rect(a, r, ox, oy, min(ox + kBigTile - 1, r.px1), min(oy + kBigTile - 1, r.py1), lane, OXC_BIG_TALLY);
  }
#endif
