// plane_hist.cpp -- plane layer: the sub-band histograms of the encoder's quantiser choice (hist.hip):
// schro_hip_histogram_batch turns the bands of every plane of a call into the jobs of one histogram_kernel launch.

#include "schro_hip_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <utility>

using namespace schro;

namespace schro {

int
histogram_batch_run (SchroHipContext * ctx, const SchroHipHistogramPlane * planes, int nplanes, int bpp, bool allow_empty)
{
  SCHRO_HIP_REQUIRE (ctx && planes && nplanes > 0, "histogram_batch: bad arguments");
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "histogram_batch: bytes_per_sample must be 2 or 4");
  (void) hipSetDevice (ctx->device);
  int group_bytes, per_tile, per_step;
  hist_tile_geometry (&group_bytes, &per_tile, &per_step);
  const int group = group_bytes / bpp;
  std::vector < HistJob > jobs;
  long long total_tiles = 0;
  // everything is validated before anything is enqueued
  for (int p = 0; p < nplanes; p++) {
    const SchroHipHistogramPlane & pl = planes[p];
    SCHRO_HIP_REQUIRE (pl.coeffs && pl.bands && pl.nbands > 0 && pl.counts && pl.bytes > 0 && (uintptr_t) pl.coeffs % bpp == 0
        && (uintptr_t) pl.counts % sizeof (uint32_t) == 0,
        "histogram_batch: plane %d invalid (coeffs, bands, counts and a size are needed, aligned to the sample)", p);
    for (int b = 0; b < pl.nbands; b++) {
      const SchroHipHistogramBand & bd = pl.bands[b];
      SCHRO_HIP_REQUIRE (bd.width >= 0 && bd.height >= 0 && (allow_empty || (bd.width > 0 && bd.height > 0)),
          "histogram_batch: plane %d band %d: %d x %d samples", p, b, bd.width, bd.height);
      if (bd.width == 0 || bd.height == 0)
        continue;
      SCHRO_HIP_REQUIRE (bd.skip >= 1 && (bd.skip & (bd.skip - 1)) == 0,
          "histogram_batch: plane %d band %d: a skip of %d (a power of two >= 1)", p, b, bd.skip);
      SCHRO_HIP_REQUIRE (bd.stride > 0 && bd.stride % bpp == 0 && (long long) bd.stride >= (long long) bd.width * bpp,
          "histogram_batch: plane %d band %d: a stride of %d bytes for rows of %d samples of %d bytes", p, b, bd.stride, bd.width, bpp);
      // (all rows of the band, the rows between the sampled ones included: the DC form reads row j - 1, and its row 0
      // reads no row above it, so a band that lies inside the plane is all either form touches)
      SCHRO_HIP_REQUIRE (bd.offset >= 0 && bd.offset % bpp == 0
          && (unsigned long long) bd.offset + (unsigned long long) (bd.height - 1) * bd.stride
          + (unsigned long long) bd.width * bpp <= (unsigned long long) pl.bytes,
          "histogram_batch: plane %d band %d (%d x %d at byte %d, pitch %d) reaches outside the plane's %zu bytes", p, b, bd.width,
          bd.height, bd.offset, bd.stride, pl.bytes);
      int shift = 0;
      while ((1 << shift) < bd.skip)
        shift++;
      const long long rows = ((long long) bd.height + bd.skip - 1) >> shift;
      SCHRO_HIP_REQUIRE (rows * bd.width < ((long long) 1 << 32),
          "histogram_batch: plane %d band %d: %lld sampled values (fewer than 2^32 are counted)", p, b, rows * bd.width);
      HistJob j;
      memset (&j, 0, sizeof (j));
      j.base = (const char *) pl.coeffs + bd.offset;
      j.counts = (uint32_t *) (pl.counts + b);
      j.stride = bd.stride;
      j.w = bd.width;
      j.skip_shift = shift;
      j.dc = bd.dc_predict != 0;
      j.gpr = (uint32_t) div_up (bd.width, group);
      j.items = (uint32_t) (rows * j.gpr);
      j.step_rows = (uint32_t) per_step / j.gpr;
      j.step_groups = (uint32_t) per_step % j.gpr;
      j.tile_base = (int) total_tiles;
      total_tiles += ((long long) j.items + per_tile - 1) / per_tile;
      SCHRO_HIP_REQUIRE (total_tiles < ((long long) 1 << 31), "histogram_batch: plane %d band %d: %lld tiles", p, b, total_tiles);
      jobs.push_back (j);
    }
  }

  // the clear: planes whose counts lie one behind the other (the frame layer's, Context.histogram_planes') share one memset --
  // a memset per plane is a dispatch per plane, 24 of them cost more than the launch
  std::vector < std::pair < uintptr_t, size_t > >clears;
  for (int p = 0; p < nplanes; p++)
    clears.emplace_back ((uintptr_t) planes[p].counts, sizeof (SchroHipHistogramCounts) * (size_t) planes[p].nbands);
  std::sort (clears.begin (), clears.end ());
  for (size_t k = 0; k < clears.size ();) {
    uintptr_t end = clears[k].first + clears[k].second;
    size_t m = k + 1;
    while (m < clears.size () && clears[m].first <= end) {
      end = std::max (end, clears[m].first + clears[m].second);
      m++;
    }
    SCHRO_HIP_CHECK (hipMemsetAsync ((void *) clears[k].first, 0, end - clears[k].first, ctx->stream));
    k = m;
  }
  if (jobs.empty ())
    return 0;
  const size_t bytes = sizeof (HistJob) * jobs.size ();
  void *d_jobs;
  int r = bytes <= SchroHipContext::kArgSlotBytes ? push_args (ctx, jobs.data (), bytes, &d_jobs)
      : push_big_table (ctx, jobs.data (), bytes, &d_jobs);
  if (r)
    return r;
  // (no profile class: SCHRO_HIP_KERNEL_CLASSES is what it was; schro_hip_timer_begin / _end time the call)
  return launch_histogram (ctx->stream, (const HistJob *) d_jobs, (int) jobs.size (), (int) total_tiles, bpp);
}

void
frame_hist_table_free (SchroHipContext * ctx)
{
  FrameHistTable *t = ctx->frame_h_table;
  if (!t)
    return;
  if (t->d_counts || t->h_counts) {
    for (int q = 0; q < SchroHipContext::kQueues; q++)  // launches and copies that still use the counts
      if (ctx->streams[q])
        (void) hipStreamSynchronize (ctx->streams[q]);
    if (t->d_counts)
      (void) hipFree (t->d_counts);
    if (t->h_counts)
      (void) hipHostFree (t->h_counts);
  }
  delete t;
  ctx->frame_h_table = nullptr;
}

}                               // namespace schro

extern "C" {

int
schro_hip_histogram_batch (SchroHipContext * ctx, const SchroHipHistogramPlane * planes, int nplanes, int bytes_per_sample)
{
  return histogram_batch_run (ctx, planes, nplanes, bytes_per_sample, false);
}

}                               // extern "C"
