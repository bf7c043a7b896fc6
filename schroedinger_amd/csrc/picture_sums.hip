// picture_sums.hip -- the sums under schro_frame_calculate_average_luma (schroframe.c:1647-1680) and
// schro_frame_mean_squared_error (schroanalysis.c:44-84): per plane the sum of its samples (orc_sum_u8, orc_sum_s16) and
// the sum of the squared differences against a second u8 plane (orc_sum_square_diff_u8, schroorc-dist.c:9361-9548).
// Integer arithmetic only, 64-bit accumulators: the sums are exact and the same bits on every run, whatever order the
// workgroups' integer atomics land in.
//
// The squared difference: the reference subtracts two zero-extended bytes in 16 bits (subw) and keeps the low 16 bits of
// the product (mullw), zero-extended (convuwl).  |a - b| <= 255 and 255^2 = 65025 < 65536, so no bit is ever lost and
// (a - b) * (a - b) in int is the same number.
//
// A workgroup of 4 waves owns a tile of kSumsTileBytes bytes of kSumsTileRows rows: a lane takes four adjacent bytes of
// a row (four u8 or two s16 samples) with one byte-aligned dword load, the lanes of the workgroup 1 KiB of the row, the
// workgroup one row after the other.  The partial sums go down the wave with shuffles, across the waves through LDS, and
// one lane adds the tile's two words to the job's result.  The result words are cleared by a launch in front.

#include "schro_hip_internal.h"

namespace schro {

constexpr int kSumsThreads = 256;
static_assert (kSumsTileBytes == kSumsThreads * 4, "a lane takes one dword of a row");

__global__ __launch_bounds__ (64)
void plane_sums_clear_kernel (const SumsJob * __restrict__ jobs, int njobs)
{
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= njobs)
    return;
  unsigned long long *r = jobs[j].result;
  gstore < unsigned long long >(r, 0ull);
  gstore < unsigned long long >(r + 1, 0ull);
}

__device__ __forceinline__ long long
sums_wave_add (long long v)
{
  for (int d = 32; d > 0; d >>= 1)
    v += __shfl_down (v, d);
  return v;
}

__global__ __launch_bounds__ (kSumsThreads)
void plane_sums_kernel (const SumsJob * __restrict__ jobs, int njobs)
{
  __shared__ long long part[2][kSumsThreads / 64];
  const int bid = blockIdx.x;
  const SumsJob job = jobs[find_job (jobs, njobs, bid)];
  const int t = bid - job.tile_base;
  const int ty = t / job.tiles_x, tx = t - ty * job.tiles_x;
  const int row_bytes = job.w * job.bps;
  const int x0 = tx * kSumsTileBytes + (int) threadIdx.x * 4;   // this lane's four bytes of a row
  const int nb = min (4, row_bytes - x0);                       // ... of which are the row's (<= 0: none)
  const int y0 = ty * kSumsTileRows, y1 = min (y0 + kSumsTileRows, job.h);

  long long sum = 0, sq = 0;
  if (nb > 0)
    for (int y = y0; y < y1; y++) {
      const uint8_t *pa = (const uint8_t *) job.a + (size_t) y * job.a_stride + x0;
      const uint8_t *pb = job.b ? job.b + (size_t) y * job.b_stride + x0 : nullptr;
      uint32_t va = 0, vb = 0;
      if (nb == 4) {
        va = gload < u32_u > (pa);
        if (pb)
          vb = gload < u32_u > (pb);
      } else
        for (int k = 0; k < nb; k++) {
          va |= (uint32_t) gload < uint8_t > (pa + k) << (8 * k);
          if (pb)
            vb |= (uint32_t) gload < uint8_t > (pb + k) << (8 * k);
        }
      if (job.bps == 1) {
        // (bytes behind the row are zero in both words: they add nothing)
        sum += (va & 255) + ((va >> 8) & 255) + ((va >> 16) & 255) + (va >> 24);
        if (pb)
          for (int k = 0; k < 4; k++) {
            const int d = (int) ((va >> (8 * k)) & 255) - (int) ((vb >> (8 * k)) & 255);
            sq += d * d;
          }
      } else
        sum += (int) (int16_t) (va & 0xffff) + (int) (int16_t) (va >> 16);      // (a row of s16 is whole samples: nb is 2 or 4)
    }

  sum = sums_wave_add (sum);
  sq = sums_wave_add (sq);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[0][wave] = sum;
    part[1][wave] = sq;
  }
  __syncthreads ();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kSumsThreads / 64; k++) {
      sum += part[0][k];
      sq += part[1][k];
    }
    // two's complement: the unsigned add of a negative sum is the signed one
    if (sum)
      atomicAdd (job.result, (unsigned long long) sum);
    if (sq)
      atomicAdd (job.result + 1, (unsigned long long) sq);
  }
}

int
launch_plane_sums (hipStream_t stream, const SumsJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH (plane_sums_clear_kernel, dim3 (div_up (njobs, 64)), dim3 (64), 0, stream, d_jobs, njobs);
  SCHRO_LAUNCH (plane_sums_kernel, dim3 (total_tiles), dim3 (kSumsThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "plane sums launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
