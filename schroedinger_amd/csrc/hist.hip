// hist.hip -- the sub-band histograms behind the encoder's quantiser choice.
//
// What it computes, per sub-band (schro_encoder_generate_subband_histograms, schroquantiser.c:600-637, over
// schro_frame_data_generate_histogram / _dc_predict, schrohistogram.c:345-391): how many of the SAMPLED values -- rows
// 0, skip, 2 skip ... of the band, all columns -- fall into each of the 104 logarithmic bins of ilogx (:11-22): |v| itself
// below 16, then 8 bins per octave.  The plain form counts the coefficient; the DC form (sub-band 0 of a picture without
// references) counts coefficient - prediction, the prediction taken from the ORIGINAL left, upper and upper-left
// neighbours (row j - 1 of the band, whatever the skip): nothing is a recurrence, every sample stands alone.  The scale
// by skip and the conversion to doubles are the host's (frame.cpp).
// One deliberate departure: the reference indexes bins[ilogx (v)] unbounded, and -32768 (index 104) or a DC difference
// beyond 15 bits (up to index 111) writes past its array; here every such sample is counted in `overflow`, the word
// behind the bins, and the bins stay as they are.  s32 frames (the reference reads s16 only): the same arithmetic in
// 32-bit wrapping ints, so that values within 16 bits give the s16 result; anything at index >= 104 is overflow.
//
// histogram_kernel: one 256-thread workgroup = 2048 consecutive 16-byte groups (8 s16 / 4 s32 samples) of one band's
// sampled rows, 8 groups per lane, all of them asked for before the first is used; all bands of all planes of a call in
// one launch (sizes, skips and forms mix: the job table).  Rows start at 2- or 4-byte alignment: a whole group is one
// 16-byte load at that alignment, a row's last columns go sample by sample; the DC form (LL bands: a few percent of a
// picture) goes sample by sample throughout.  Counts: one private histogram per wave in LDS (104 + 1 words, LDS atomics);
// the lowest kHot bins -- where most wavelet coefficients fall, so that most lanes of a wave would meet on one LDS word and
// be served one after the other -- are counted in registers of the lane's own instead (a byte per bin) and summed over
// the wave once, at the end.  The four waves merge through LDS, then one global atomic add per non-empty bin per workgroup into counts the
// call has cleared: unsigned integers, so the result is exact whatever the order.  Measured: wavelet coefficients and values
// uniform over s16 take the same time, 2.7 x the byte floor of the sampled rows (2.9 TB/s) -- neither the bytes nor the
// LDS atomics alone bound it; what fills the rest (about 20 vector instructions per sample, the per-workgroup clear, probe
// and merge) has not been traced.

#include "schro_hip_internal.h"

#include <cstdlib>

namespace schro {
namespace {

constexpr int kHThreads = 256, kHWaves = kHThreads / 64, kHItems = 8, kHSlots = SCHRO_HIP_HISTOGRAM_BINS + 1;
constexpr int kHot = 4;

// ilogx of |v|, 104 (the overflow slot) for everything from 2^15 up
__device__ __forceinline__ uint32_t
hist_slot (int32_t v)
{
  const uint32_t x = v < 0 ? 0u - (uint32_t) v : (uint32_t) v;
  const int i = max (0, 28 - (int) __clz ((int) x));    // halvings until x < 16 (__clz (0) is 32)
  return min ((x >> i) + 8u * (uint32_t) i, (uint32_t) SCHRO_HIP_HISTOGRAM_BINS);
}

// one sample of a lane (valid: the lane has one).  Slots below HOT (0, 4 or 8) go to the lane's own counters, a byte
// each -- a lane sees kHItems x 8 = 64 samples at the most --, every other slot to the wave's histogram in LDS.
template < int HOT >
__device__ __forceinline__ void
hist_count (uint32_t * wave_hist, uint32_t (&hot)[HOT ? HOT / 4 : 1], uint32_t slot, bool valid)
{
  const uint32_t one = 1u << ((slot & 3u) * 8u);
#pragma unroll
  for (int r = 0; r < HOT / 4; r++)
    hot[r] += valid && (slot >> 2) == (uint32_t) r ? one : 0u;
  if (valid && slot >= (uint32_t) HOT)
    __hip_atomic_fetch_add (&wave_hist[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the lanes' counters summed over the wave (16-bit fields: 64 lanes x 64 samples fit) and added to its histogram
template < int HOT >
__device__ __forceinline__ void
hist_flush_hot (uint32_t * wave_hist, const uint32_t (&hot)[HOT ? HOT / 4 : 1], int lane)
{
#pragma unroll
  for (int r = 0; r < HOT / 4; r++) {
    uint32_t even = hot[r] & 0x00ff00ffu, odd = (hot[r] >> 8) & 0x00ff00ffu;    // slots 4 r + 0, 2 and 4 r + 1, 3
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      even += (uint32_t) __shfl_xor ((int) even, o);
      odd += (uint32_t) __shfl_xor ((int) odd, o);
    }
    if (lane < 4) {
      const uint32_t f = lane & 1 ? odd : even;
      const uint32_t c = lane & 2 ? f >> 16 : f & 0xffffu;
      if (c)
        __hip_atomic_fetch_add (&wave_hist[4 * r + lane], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}

template < typename T >
__device__ __forceinline__ int32_t
group_sample (const u32x4 & raw, int e)
{
  if constexpr (sizeof (T) == 2)
    return (int16_t) (raw[e >> 1] >> (16 * (e & 1)));
  else
    return (int32_t) raw[e];
}

template < typename T, int HOT >
__global__ __launch_bounds__ (kHThreads)
void histogram_kernel (const HistJob * __restrict__ jobs, int njobs)
{
  constexpr int G = 16 / (int) sizeof (T);
  __shared__ uint32_t hist[kHWaves][kHSlots];
  const int bid = blockIdx.x, tid = threadIdx.x;
  const HistJob job = jobs[find_job (jobs, njobs, bid)];
  for (int s = tid; s < kHWaves * kHSlots; s += kHThreads)
    (&hist[0][0])[s] = 0;
  __syncthreads ();
  uint32_t *const wave_hist = hist[tid >> 6];
  uint32_t hot[HOT ? HOT / 4 : 1] = { };
  // this workgroup's groups: `first` .. of the band's rows x groups-per-row; lane tid takes first + tid + 256 k
  const uint32_t first = (uint32_t) (bid - job.tile_base) * (uint32_t) (kHThreads * kHItems);
  const uint32_t remaining = job.items - first;
  uint32_t g = first % job.gpr + (uint32_t) tid, row = first / job.gpr + g / job.gpr;
  g %= job.gpr;
  auto line_of = [&] (uint32_t r)->const T * {
    return (const T *) ((const char *) job.base + ((size_t) r << job.skip_shift) * (size_t) job.stride);
  };
  auto advance = [&] () {
    g += job.step_groups;
    row += job.step_rows;
    if (g >= job.gpr) {
      g -= job.gpr;
      row++;
    }
  };
  if (!job.dc) {
    // whole groups first: one 16-byte load each, all asked for before the first is counted ...
    const uint32_t g0 = g, row0 = row;
    const int tail = job.w % G;         // samples of a row's last group, 0: it is whole
    u32x4 raw[kHItems];
    uint32_t whole = 0;
#pragma unroll
    for (int k = 0; k < kHItems; k++) {
      raw[k] = (u32x4) { 0, 0, 0, 0 };
      if ((uint32_t) (tid + k * kHThreads) < remaining && (tail == 0 || g + 1 < job.gpr)) {
        raw[k] = gload < u32x4_u > (line_of (row) + (int) g * G);
        whole |= 1u << k;
      }
      advance ();
    }
#pragma unroll
    for (int k = 0; k < kHItems; k++) {
      if (whole & (1u << k)) {
#pragma unroll
        for (int e = 0; e < G; e++)
          hist_count < HOT > (wave_hist, hot, hist_slot (group_sample < T > (raw[k], e)), true);
      }
    }
    // ... then the ragged ends, sample by sample: the last group of a row whose width is no multiple of the group
    if (tail) {
      g = g0;
      row = row0;
#pragma unroll 1
      for (int k = 0; k < kHItems; k++) {
        if ((uint32_t) (tid + k * kHThreads) < remaining && g + 1 == job.gpr) {
          const T *p = line_of (row) + (int) g * G;
#pragma unroll
          for (int e = 0; e < G - 1; e++)
            if (e < tail)
              hist_count < HOT > (wave_hist, hot, hist_slot (gload < T > (p + e)), true);
        }
        advance ();
      }
    }
  } else {
    // (the arithmetic is uint32_t where C's int would overflow on s32 samples; on s16 samples nothing wraps)
#pragma unroll 1
    for (int k = 0; k < kHItems; k++) {
      int32_t v[G];
      int n = 0;
#pragma unroll
      for (int e = 0; e < G; e++)
        v[e] = 0;
      if ((uint32_t) (tid + k * kHThreads) < remaining) {
        const int x = (int) g * G;
        const bool top = row == 0;      // (row 0 of the sampled rows is row 0 of the band)
        const T *line = line_of (row) + x;
        const T *prev = (const T *) ((const char *) line - job.stride);         // row j - 1 of the band; never read when top
        n = min (G, job.w - x);
        int32_t left = x > 0 ? (int32_t) gload < T > (line - 1) : 0;
        int32_t upleft = x > 0 && !top ? (int32_t) gload < T > (prev - 1) : 0;
#pragma unroll
        for (int e = 0; e < G; e++)
          if (e < n) {
            const int32_t cur = gload < T > (line + e);
            const int32_t up = top ? 0 : (int32_t) gload < T > (prev + e);
            int32_t pred;
            if (!top) {
              if (x + e > 0) {
                const uint32_t a = (uint32_t) left + (uint32_t) up + (uint32_t) upleft + 1u;
                pred = (int32_t) (a * 21845u + 10922u) >> 16;   // schro_divide3
              } else {
                pred = up;
              }
            } else {
              pred = x + e > 0 ? left : 0;
            }
            v[e] = (int32_t) ((uint32_t) cur - (uint32_t) pred);
            left = cur;
            upleft = up;
          }
      }
#pragma unroll
      for (int e = 0; e < G; e++)
        hist_count < HOT > (wave_hist, hot, hist_slot (v[e]), e < n);
      advance ();
    }
  }
  hist_flush_hot < HOT > (wave_hist, hot, tid & 63);
  __syncthreads ();
  if (tid < kHSlots) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kHWaves; w++)
      sum += hist[w][tid];
    if (sum)
      __hip_atomic_fetch_add ((SCHRO_GLOBAL uint32_t *) (job.counts + tid), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}                               // namespace

void
hist_tile_geometry (int *group_bytes, int *groups_per_tile, int *groups_per_step)
{
  *group_bytes = 16;
  *groups_per_tile = kHThreads * kHItems;
  *groups_per_step = kHThreads;
}

template < typename T >
static void
launch_histogram_as (int hot, hipStream_t stream, const HistJob * d_jobs, int njobs, int total_tiles)
{
#ifdef SCHRO_HIP_EXPERIMENTS
  // A/B (scripts/histogram_ab.py): how many of the lowest bins are counted in registers (0, 4, 8); 0: every sample an LDS atomic
  if (hot == 0)
    SCHRO_LAUNCH ((histogram_kernel < T, 0 >), dim3 (total_tiles), dim3 (kHThreads), 0, stream, d_jobs, njobs);
  else if (hot == 8)
    SCHRO_LAUNCH ((histogram_kernel < T, 8 >), dim3 (total_tiles), dim3 (kHThreads), 0, stream, d_jobs, njobs);
  else
#endif
    SCHRO_LAUNCH ((histogram_kernel < T, kHot >), dim3 (total_tiles), dim3 (kHThreads), 0, stream, d_jobs, njobs);
  (void) hot;
}

int
launch_histogram (hipStream_t stream, const HistJob * d_jobs, int njobs, int total_tiles, int bpp)
{
  const int hot = SCHRO_ENV ("SCHRO_HIP_HIST_HOT") ? atoi (SCHRO_ENV ("SCHRO_HIP_HIST_HOT")) : kHot;
  if (bpp == 2)
    launch_histogram_as < int16_t > (hot, stream, d_jobs, njobs, total_tiles);
  else
    launch_histogram_as < int32_t > (hot, stream, d_jobs, njobs, total_tiles);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "histogram launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
