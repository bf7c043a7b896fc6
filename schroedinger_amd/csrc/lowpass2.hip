// lowpass2.hip -- schro_frame_component_filter_lowpass2_u8 / _s16 (schrofilter.c:516-782): the recursive Gaussian of
// schro_frame_filter_lowpass2, which is the encoder's pre-filter `filtering = 2` and, five times, schro_frame_ssim.
//
// A plane is filtered IN PLACE by four passes, each rounded to the sample type before the next reads it: every row
// forward (start state s[0], three times), every row in reverse (start state d[n - 1] as the forward pass stored it),
// the columns forward (start state row 0 as the rows left it), the columns in reverse (start state the last row as the
// forward column pass left it).  One step is
//     x = c0 * s + c1 * i0 + c2 * i1 + c3 * i2;  i2 = i1;  i1 = i0;  i0 = x;  d = rint (x)
// in IEEE double, left to right: four rounded products and three rounded sums, as the reference's x86-64 build (SSE2)
// evaluates it.  hipcc would contract the products into the sums (FMA), which changes the last bit of x and, through
// rint, samples; contraction is switched off for this file by the pragma below.  The state carries the UNROUNDED x.
//
// Out of range: `d[i] = rint (x)` with d a uint8_t / int16_t converts the double to int32 (cvttsd2si) and stores the low
// 8 / 16 bits in that build; a double outside int32 converts to INT_MIN.  lowpass_step does the same and counts every
// sample whose int32 value is not the stored one.
//
// The recursion is serial along a row and parallel over rows, then serial down a column and parallel over columns.
//   lowpass_rows_kernel: one wave owns kLowpassRows rows.  It walks them in chunks of kLowpassChunk columns: the chunk of
//     all its rows is staged in LDS with the lanes along the row (coalesced), each lane then walks ITS row's chunk in LDS
//     (the row pitch is an odd number of dwords: the lanes' samples sit in different banks), and the chunk is written
//     back the way it came.  The three doubles of the state stay in the lane's registers from chunk to chunk, so the
//     recursion crosses chunk borders exactly; the reverse pass takes the chunks from the last to the first.
//   lowpass_cols_kernel: one wave owns kLowpassCols columns, a lane one column: the loads and stores of a row are
//     coalesced as they stand.  kLowpassColRows rows are loaded at a time so that their latencies overlap.

#include "schro_hip_internal.h"

#include <climits>

#pragma clang fp contract(off)

namespace schro {

constexpr int kLowpassThreads = 64;
static_assert (kLowpassRows == kLowpassThreads && kLowpassCols == kLowpassThreads, "a lane owns a row, then a column");

template < typename T > __device__ __forceinline__ T
lowpass_step (double s, const double *c, double &i0, double &i1, double &i2, uint32_t & bad)
{
  const double x = c[0] * s + c[1] * i0 + c[2] * i1 + c[3] * i2;
  i2 = i1;
  i1 = i0;
  i0 = x;
  const double r = rint (x);
  // cvttsd2si: the "integer indefinite" value for what int32 does not hold (NaN included)
  const int v = (r >= -2147483648.0 && r < 2147483648.0) ? (int) r : INT_MIN;
  const T d = (T) v;            // the low 8 / 16 bits
  bad += (int) d != v;
  return d;
}

__device__ __forceinline__ void
lowpass_count (uint32_t * counter, uint32_t bad)
{
  for (int d = 32; d > 0; d >>= 1)
    bad += __shfl_down (bad, d);
  if ((threadIdx.x & 63) == 0 && bad)
    atomicAdd (counter, bad);
}

// which job owns group `bid` of a kernel whose first groups are the jobs' `base` members (ascending from 0)
__device__ __forceinline__ int
lowpass_find (const LowpassJob * jobs, int njobs, int bid, int LowpassJob::*base)
{
  const int lane = threadIdx.x & 63;
  int n = 0;
  for (int first = 0; first < njobs; first += 64) {
    const int idx = first + lane;
    const bool le = idx < njobs && gload < int > (&(jobs[idx].*base)) <= bid;
    n += __popcll (__ballot (le));
  }
  return __builtin_amdgcn_readfirstlane (n - 1);
}

template < typename T > __device__ __forceinline__ void
lowpass_rows (const LowpassJob & job, int group, T * tile)
{
  constexpr int kPitch = kLowpassChunk + 4 / (int) sizeof (T); // an odd number of dwords
  const int lane = threadIdx.x;
  const int y0 = group * kLowpassRows, rows = min (kLowpassRows, job.h - y0), w = job.w;
  char *base = (char *) job.data + (size_t) y0 * job.stride;
  const bool mine = lane < rows;
  const int nchunks = (w + kLowpassChunk - 1) / kLowpassChunk;
  T *row = tile + lane * kPitch;
  double i0 = 0, i1 = 0, i2 = 0;
  uint32_t bad = 0;

  for (int pass = 0; pass < 2; pass++)
    for (int cc = 0; cc < nchunks; cc++) {
      const int c = pass ? nchunks - 1 - cc : cc;
      const int x0 = c * kLowpassChunk, n = min (kLowpassChunk, w - x0);
      for (int r = 0; r < rows; r++) {
        const T *src = (const T *) (base + (size_t) r * job.stride) + x0;
        for (int x = lane; x < n; x += kLowpassThreads)
          tile[r * kPitch + x] = gload < T > (src + x);
      }
      __syncthreads ();
      if (mine) {
        if (cc == 0)
          i0 = i1 = i2 = (double) row[pass ? n - 1 : 0];
        if (!pass)
          for (int x = 0; x < n; x++)
            row[x] = lowpass_step < T > ((double) row[x], job.hc, i0, i1, i2, bad);
        else
          for (int x = n - 1; x >= 0; x--)
            row[x] = lowpass_step < T > ((double) row[x], job.hc, i0, i1, i2, bad);
      }
      __syncthreads ();
      for (int r = 0; r < rows; r++) {
        T *dst = (T *) (base + (size_t) r * job.stride) + x0;
        for (int x = lane; x < n; x += kLowpassThreads)
          gstore < T > (dst + x, tile[r * kPitch + x]);
      }
      // the reverse pass reads what the forward pass stored; the next chunk overwrites the tile
      __threadfence_block ();
      __syncthreads ();
    }
  lowpass_count (job.out_of_range, bad);
}

__global__ __launch_bounds__ (kLowpassThreads)
void lowpass_rows_kernel (const LowpassJob * __restrict__ jobs, int njobs)
{
  __shared__ __attribute__ ((aligned (16))) uint32_t tile[kLowpassRows * (kLowpassChunk * 2 + 4) / 4];
  const LowpassJob job = jobs[lowpass_find (jobs, njobs, blockIdx.x, &LowpassJob::row_base)];
  const int group = blockIdx.x - job.row_base;
  if (job.bps == 1)
    lowpass_rows < uint8_t > (job, group, (uint8_t *) tile);
  else
    lowpass_rows < int16_t > (job, group, (int16_t *) tile);
}

template < typename T > __device__ __forceinline__ void
lowpass_cols (const LowpassJob & job, int group)
{
  const int x = group * kLowpassCols + (int) threadIdx.x, h = job.h;
  uint32_t bad = 0;
  if (x < job.w) {
    char *col = (char *) job.data + (size_t) x * sizeof (T);
    T v[kLowpassColRows];
    double i0, i1, i2;
    i0 = i1 = i2 = (double) gload < T > (col);
    for (int y0 = 0; y0 < h; y0 += kLowpassColRows) {
      const int n = min (kLowpassColRows, h - y0);
#pragma unroll
      for (int k = 0; k < kLowpassColRows; k++)
        if (k < n)
          v[k] = gload < T > (col + (size_t) (y0 + k) * job.stride);
#pragma unroll
      for (int k = 0; k < kLowpassColRows; k++)
        if (k < n)
          gstore < T > (col + (size_t) (y0 + k) * job.stride, lowpass_step < T > ((double) v[k], job.vc, i0, i1, i2, bad));
    }
    __threadfence_block ();     // (the lane reads its own stores back)
    i0 = i1 = i2 = (double) gload < T > (col + (size_t) (h - 1) * job.stride);
    for (int y1 = h; y1 > 0; y1 -= kLowpassColRows) {
      const int n = min (kLowpassColRows, y1);
#pragma unroll
      for (int k = 0; k < kLowpassColRows; k++)
        if (k < n)
          v[k] = gload < T > (col + (size_t) (y1 - 1 - k) * job.stride);
#pragma unroll
      for (int k = 0; k < kLowpassColRows; k++)
        if (k < n)
          gstore < T > (col + (size_t) (y1 - 1 - k) * job.stride, lowpass_step < T > ((double) v[k], job.vc, i0, i1, i2, bad));
    }
  }
  lowpass_count (job.out_of_range, bad);
}

__global__ __launch_bounds__ (kLowpassThreads)
void lowpass_cols_kernel (const LowpassJob * __restrict__ jobs, int njobs)
{
  const LowpassJob job = jobs[lowpass_find (jobs, njobs, blockIdx.x, &LowpassJob::col_base)];
  const int group = blockIdx.x - job.col_base;
  if (job.bps == 1)
    lowpass_cols < uint8_t > (job, group);
  else
    lowpass_cols < int16_t > (job, group);
}

int
launch_lowpass2 (hipStream_t stream, const LowpassJob * d_jobs, int njobs, int row_groups, int col_groups)
{
  SCHRO_LAUNCH (lowpass_rows_kernel, dim3 (row_groups), dim3 (kLowpassThreads), 0, stream, d_jobs, njobs);
  SCHRO_LAUNCH (lowpass_cols_kernel, dim3 (col_groups), dim3 (kLowpassThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "lowpass2 launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
