// ssim.hip -- what schro_frame_ssim (schrossim.c:64-149) reads, around the five low-passes of lowpass2.hip.
//
// Only the luma planes: the reference filters the chroma too and never looks at it.  In the reference's order:
//   ssim_prepare_kernel   a_lowpass = a, b_lowpass = b (the copies schro_frame_dup makes for the in-place low-pass); the
//                         result's counters are cleared here
//   (low-pass of a_lowpass, b_lowpass as u8)
//   ssim_products_kernel  a_hipass = (a - 128) - a_lowpass, b_hipass = (b - 128) - b_lowpass in s16 (schro_frame_dup16
//                         converts u8 to s16 with orc_offsetconvert_s16_u8, schroframe.c:917, schrovirtframe.c:1742-1750;
//                         then schro_frame_subtract), then ab, a^2, b^2 = CLAMP (int product, -32768, 32767)
//                         (schro_frame_multiply_s16, :49-50): the difference, the product and the clamp in one pass
//   (low-pass of ab, a^2, b^2 as s16)
//   ssim_final_kernel     the per-pixel expression (:116-117), the integer terms in int, the rest in double, left to right
//                         and without contraction (the pragma below); the value goes to the map and into the sum
//   ssim_sum_kernel       the tiles' partial sums in a fixed order
//
// The sum cannot be the reference's single raster-order accumulator.  It is deterministic instead, without
// floating-point atomics: a lane adds its column of the tile's kSsimTileRows rows from the top, the lanes of a wave and
// then the waves are added in a fixed tree, the tile's sum is stored, and one workgroup per picture adds the tiles' sums
// (lane i takes tiles i, i + 256, ... in order, then the same tree).

#include "schro_hip_internal.h"

#pragma clang fp contract(off)

namespace schro {

constexpr int kSsimThreads = 256;
static_assert (kSsimTileCols == kSsimThreads, "a lane owns a column of the tile");

struct SsimTile {
  int x, y0, y1;
  bool in;
  int tile;
};

__device__ __forceinline__ SsimTile
ssim_tile (const SsimJob & job, int bid)
{
  SsimTile t;
  t.tile = bid - job.tile_base;
  const int ty = t.tile / job.tiles_x, tx = t.tile - ty * job.tiles_x;
  t.x = tx * kSsimTileCols + (int) threadIdx.x;
  t.y0 = ty * kSsimTileRows;
  t.y1 = min (t.y0 + kSsimTileRows, job.h);
  t.in = t.x < job.w;
  return t;
}

__global__ __launch_bounds__ (kSsimThreads)
void ssim_prepare_kernel (const SsimJob * __restrict__ jobs, int njobs)
{
  const SsimJob job = jobs[find_job (jobs, njobs, blockIdx.x)];
  const SsimTile t = ssim_tile (job, blockIdx.x);
  if (t.tile == 0 && threadIdx.x < 8)
    gstore < uint32_t > ((uint32_t *) job.result + threadIdx.x, 0u);      // sum, out_of_range[5], reserved
  if (!t.in)
    return;
  for (int y = t.y0; y < t.y1; y++) {
    gstore < uint8_t > (job.a_low + (size_t) y * job.stride8 + t.x, gload < uint8_t > (job.a + (size_t) y * job.a_stride + t.x));
    gstore < uint8_t > (job.b_low + (size_t) y * job.stride8 + t.x, gload < uint8_t > (job.b + (size_t) y * job.b_stride + t.x));
  }
}

__device__ __forceinline__ int16_t
ssim_clamp (int z)
{
  return (int16_t) min (max (z, -32768), 32767);
}

__global__ __launch_bounds__ (kSsimThreads)
void ssim_products_kernel (const SsimJob * __restrict__ jobs, int njobs)
{
  const SsimJob job = jobs[find_job (jobs, njobs, blockIdx.x)];
  const SsimTile t = ssim_tile (job, blockIdx.x);
  if (!t.in)
    return;
  for (int y = t.y0; y < t.y1; y++) {
    // schro_frame_dup16 is schro_frame_convert into s16, which takes 128 off a u8 sample (orc_offsetconvert_s16_u8);
    // schro_frame_subtract then takes the u8 low-pass off that: -383 .. 127, so the products reach 146689 and the clamp bites
    const int ah = (int) gload < uint8_t > (job.a + (size_t) y * job.a_stride + t.x) - 128 - (int) gload < uint8_t > (job.a_low + (size_t) y * job.stride8 + t.x);
    const int bh = (int) gload < uint8_t > (job.b + (size_t) y * job.b_stride + t.x) - 128 - (int) gload < uint8_t > (job.b_low + (size_t) y * job.stride8 + t.x);
    const size_t o = (size_t) y * job.stride16 + (size_t) t.x * 2;
    gstore < int16_t > ((char *) job.ab + o, ssim_clamp (ah * bh));
    gstore < int16_t > ((char *) job.aa + o, ssim_clamp (ah * ah));
    gstore < int16_t > ((char *) job.bb + o, ssim_clamp (bh * bh));
  }
}

// the sum of the workgroup's 256 values in a fixed tree (valid in thread 0)
__device__ __forceinline__ double
ssim_tree (double v, double *part)
{
  for (int d = 32; d > 0; d >>= 1)
    v = v + __shfl_down (v, d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
    part[wave] = v;
  __syncthreads ();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__ (kSsimThreads)
void ssim_final_kernel (const SsimJob * __restrict__ jobs, int njobs)
{
  __shared__ double part[kSsimThreads / 64];
  const SsimJob job = jobs[find_job (jobs, njobs, blockIdx.x)];
  const SsimTile t = ssim_tile (job, blockIdx.x);
  const double c1 = (0.01 * 255) * (0.01 * 255);
  const double c2 = (0.03 * 255) * (0.03 * 255);
  double sum = 0;
  if (t.in)
    for (int y = t.y0; y < t.y1; y++) {
      const size_t o8 = (size_t) y * job.stride8 + t.x, o16 = (size_t) y * job.stride16 + (size_t) t.x * 2;
      const int mu_x = gload < uint8_t > (job.a_low + o8), mu_y = gload < uint8_t > (job.b_low + o8);
      const int sigma_x2 = gload < int16_t > ((const char *) job.aa + o16), sigma_y2 = gload < int16_t > ((const char *) job.bb + o16);
      const int sigma_xy = gload < int16_t > ((const char *) job.ab + o16);
      const double ssim = (2 * mu_x * mu_y + c1) * (2 * sigma_xy + c2) / ((mu_x * mu_x + mu_y * mu_y + c1) * (sigma_x2 + sigma_y2 + c2));
      if (job.map)
        gstore < double >((char *) job.map + (size_t) y * job.map_stride + (size_t) t.x * 8, ssim);
      sum = sum + ssim;
    }
  sum = ssim_tree (sum, part);
  if (threadIdx.x == 0)
    gstore < double >(job.partial + t.tile, sum);
}

__global__ __launch_bounds__ (kSsimThreads)
void ssim_sum_kernel (const SsimJob * __restrict__ jobs)
{
  __shared__ double part[kSsimThreads / 64];
  const SsimJob job = jobs[blockIdx.x];
  double sum = 0;
  for (int k = threadIdx.x; k < job.ntiles; k += kSsimThreads)
    sum = sum + gload < double >(job.partial + k);
  sum = ssim_tree (sum, part);
  if (threadIdx.x == 0)
    gstore < double >(&job.result->sum, sum);
}

static int
ssim_launched (const char *what)
{
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "ssim %s launch: %s", what, hipGetErrorString (e));
  return 0;
}

int
launch_ssim_prepare (hipStream_t stream, const SsimJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH (ssim_prepare_kernel, dim3 (total_tiles), dim3 (kSsimThreads), 0, stream, d_jobs, njobs);
  return ssim_launched ("prepare");
}

int
launch_ssim_products (hipStream_t stream, const SsimJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH (ssim_products_kernel, dim3 (total_tiles), dim3 (kSsimThreads), 0, stream, d_jobs, njobs);
  return ssim_launched ("products");
}

int
launch_ssim_final (hipStream_t stream, const SsimJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH (ssim_final_kernel, dim3 (total_tiles), dim3 (kSsimThreads), 0, stream, d_jobs, njobs);
  SCHRO_LAUNCH (ssim_sum_kernel, dim3 (njobs), dim3 (kSsimThreads), 0, stream, d_jobs);
  return ssim_launched ("final");
}

}                               // namespace schro
