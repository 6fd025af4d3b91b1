// oxcull_eye_adaptation.hip -- the luminance histogram of the lit HDR image and the auto-exposure it gives (gfx950):
// RendererInstance::apply_eye_adaptation (Oxylus/src/Render/Passes/PostProcess.cpp:7-77, passes/histogram_generate.slang and
// passes/histogram_average.slang) as three launches.  Rules: include/oxcull.h, oxc_apply_eye_adaptation; design and measurements: DESIGN.md
// section 17.
//
//   k_luminance_histogram  about one resident round of blocks.  The image is one run of `pixels` texels, so a block walks it as 16-byte
//                 vectors (four B10G11R11 texels, two RGBA16F texels) in a grid-stride loop; the texels before the first 16-byte boundary and
//                 behind the last whole vector (at most three and three) are taken one by one by the first threads of block 0.
//                 - Every wave counts into its own 256-bin histogram in LDS, one LDS add per texel: no wave waits for another one's bin.
//                   Counting the lanes of a wave that share a bin with a ballot first, so that one lane adds for all of them, was measured
//                   and dropped: slower on a lit frame, a little faster only on a constant image.
//                 - One flush per block: the four wave histograms are summed per bin and the non-zero sums added to the output with one
//                   memory-side atomic each (at most 256 per block; a real frame fills a few dozen bins).
//   k_zero_histogram       zeroes the output before it, in-stream: a kernel, because a captured memset node does not replay (DESIGN.md
//                 section 15).
//   k_luminance_average    one block of 256 threads, steps 6-9: the weighted sum through LDS, then thread 0 alone.
//
// Every float operation keeps the order and rounding the header states: the file is compiled without contraction, division is the IEEE one,
// log2 / exp2 are the closed forms in binary64 of oxcull_pixel_device.hpp.  The wave's FP16 denormal mode stays at its default (RGBA16F
// holds denormal halves).
#include <hip/hip_runtime.h>

#include "oxcull_kernels.hpp"
#include "oxcull_pixel_device.hpp"

namespace oxc {

namespace {
constexpr uint32_t kBins = 256;          // GPU::HISTOGRAM_BIN_COUNT
constexpr uint32_t kQuietNaN = 0x7FC00000u;

// steps 2-4: the bin of one texel's three channels
OXC_DEV uint32_t luminance_bin(float r, float g, float b, float min_exposure, float exposure_range) {
  const float luminance = (r * 0.2127f + g * 0.7152f) + b * 0.0722f;
  if (luminance < 0.001f) return 0u;
  const float l = (float)log2_f64(luminance);
  const float mapped = ((l - min_exposure) / exposure_range) * 254.0f + 1.0f;
  return (uint32_t)clamp_i(cvt_i32_sat(mapped), 0, (int)kBins - 1);
}

// step 1 for one texel: B10G11R11 in `lo` (FORMAT 0), or the four halves of an R16G16B16A16 texel in `lo`, `hi` (FORMAT 1)
template <int FORMAT>
OXC_DEV uint32_t texel_bin(uint32_t lo, uint32_t hi, float min_exposure, float exposure_range) {
  if (FORMAT == 0) return luminance_bin(unpack_ufloat<6>(lo & 0x7FFu), unpack_ufloat<6>((lo >> 11) & 0x7FFu), unpack_ufloat<5>(lo >> 22), min_exposure, exposure_range);
  return luminance_bin(dequantize_half(lo & 0xFFFFu), dequantize_half(lo >> 16), dequantize_half(hi & 0xFFFFu), min_exposure, exposure_range);
}

// step 5 for one texel
OXC_DEV void count(uint32_t* hist, uint32_t bin) { atomicAdd(&hist[bin], 1u); }
}  // namespace

template <int FORMAT>
__global__ __launch_bounds__(256) void k_luminance_histogram(EyeAdaptationArgs a) {
  __shared__ uint32_t s_hist[4][kBins];
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; k++) s_hist[k][tid] = 0u;
  __syncthreads();
  uint32_t* const mine = s_hist[tid >> 6];
  constexpr uint32_t kPerVector = FORMAT == 0 ? 4u : 2u;  // texels in 16 bytes
  constexpr uint32_t kWords = FORMAT == 0 ? 1u : 2u;      // u32 words per texel
  const uint32_t* const words = static_cast<const uint32_t*>(a.src);

  // whole vectors: texels [head, head + vectors * kPerVector)
  const uint4* const body = reinterpret_cast<const uint4*>(words + (size_t)a.head * kWords);
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + tid; i < a.vectors; i += stride) {
    const uint4 v = body[i];
    if (FORMAT == 0) {
      count(mine, texel_bin<0>(v.x, 0u, a.min_exposure, a.exposure_range));
      count(mine, texel_bin<0>(v.y, 0u, a.min_exposure, a.exposure_range));
      count(mine, texel_bin<0>(v.z, 0u, a.min_exposure, a.exposure_range));
      count(mine, texel_bin<0>(v.w, 0u, a.min_exposure, a.exposure_range));
    } else {
      count(mine, texel_bin<1>(v.x, v.y, a.min_exposure, a.exposure_range));
      count(mine, texel_bin<1>(v.z, v.w, a.min_exposure, a.exposure_range));
    }
  }

  // the texels before and behind the vectors: at most 2 * (kPerVector - 1), one per thread of block 0
  if (blockIdx.x == 0u) {
    const uint64_t body_end = (uint64_t)a.head + a.vectors * kPerVector;
    const uint32_t tail = (uint32_t)(a.pixels - body_end);
    if (tid < a.head + tail) {
      const uint64_t p = tid < a.head ? (uint64_t)tid : body_end + (tid - a.head);
      count(mine, texel_bin<FORMAT>(words[p * kWords], FORMAT == 1 ? words[p * kWords + 1u] : 0u, a.min_exposure, a.exposure_range));
    }
  }
  __syncthreads();

  const uint32_t total = (s_hist[0][tid] + s_hist[1][tid]) + (s_hist[2][tid] + s_hist[3][tid]);
  if (total) atomicAdd(&a.histogram[tid], total);
}

// Not hipMemsetAsync: a memset node captured into a HIP graph zero-fills on the first replay only
__global__ __launch_bounds__(256) void k_zero_histogram(uint32_t* __restrict__ histogram) { histogram[threadIdx.x] = 0u; }

// steps 6-9
__global__ __launch_bounds__(256) void k_luminance_average(EyeAdaptationArgs a) {
  __shared__ uint32_t s_weighted_sum;
  const uint32_t tid = threadIdx.x;
  if (tid == 0u) s_weighted_sum = 0u;
  __syncthreads();
  const uint32_t count = a.histogram[tid];
  if (count && tid) atomicAdd(&s_weighted_sum, count * tid);  // modulo 2^32
  __syncthreads();
  if (tid != 0u) return;
  const float dark = (float)count;  // histogram[0]
  const float avg = (float)s_weighted_sum / fmaxf(a.pixel_count - dark, 1.0f) - 1.0f;
  const float desired = exp2_rule(((avg / 254.0f) * a.exposure_range) + a.min_exposure);
  const float last = a.exposure[0];
  const float adapted = last + (desired - last) * a.time_coeff;
  const float ev100 = (float)log2_f64(adapted * ((100.0f * a.ev100_bias) / 12.5f));
  const float exposure = 1.0f / (exp2_rule(ev100) * 1.2f);
  uint32_t* const out = reinterpret_cast<uint32_t*>(a.exposure);
  out[0] = adapted == adapted ? asu(adapted) : kQuietNaN;
  out[1] = exposure == exposure ? asu(exposure) : kQuietNaN;
}

void launch_eye_adaptation(const EyeAdaptationArgs& a, uint32_t grid, hipStream_t s) {
  hipLaunchKernelGGL(k_zero_histogram, dim3(1), dim3(256), 0, s, a.histogram);
  if (a.format == 0u)
    hipLaunchKernelGGL((k_luminance_histogram<0>), dim3(grid), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((k_luminance_histogram<1>), dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_luminance_average, dim3(1), dim3(256), 0, s, a);
}

}  // namespace oxc
