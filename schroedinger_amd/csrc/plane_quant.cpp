// plane_quant.cpp -- plane layer: the encoder's quantisation (quant.hip): schro_hip_quantise_batch turns codeblock
// records into the jobs of one quantise_kernel launch and, for intra pictures, the bands of one quantise_dc_kernel launch.

#include "schro_hip_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace schro {

int
quantise_batch_run (SchroHipContext * ctx, const SchroHipQuantPlane * planes, int nplanes, int bpp, bool allow_empty,
    const int32_t * const *chosen, uint32_t * clamped)
{
  SCHRO_HIP_REQUIRE (ctx && planes && nplanes > 0, "quantise_batch: bad arguments");
  // the chosen form (schro_hip_quantise_chosen_batch): a record's quant_index is its SUB-BAND, the index comes from
  // chosen[plane][sub-band] on the device -- the constants are left to a resolve launch behind the table's upload
  if (chosen) {
    SCHRO_HIP_REQUIRE (clamped && (uintptr_t) clamped % sizeof (uint32_t) == 0, "quantise_chosen_batch: clamped is NULL or not 4-byte aligned");
    for (int p = 0; p < nplanes; p++)
      SCHRO_HIP_REQUIRE (chosen[p] && (uintptr_t) chosen[p] % sizeof (int32_t) == 0,
          "quantise_chosen_batch: plane %d: chosen is NULL or not 4-byte aligned", p);
  }
  std::vector < QuantChosen > job_runs, dc_runs;
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "quantise_batch: bytes_per_sample must be 2 or 4");
  (void) hipSetDevice (ctx->device);
  int tw, th;
  quant_tile_geometry (&tw, &th);
  std::vector < QuantJob > jobs;
  std::vector < QuantDcJob > dc_jobs;
  std::vector < QuantDcRec > dc_recs;
  int dc_max_rows = 0;
  long long total_tiles = 0;
  // everything is validated before anything is enqueued
  for (int p = 0; p < nplanes; p++) {
    const SchroHipQuantPlane & pl = planes[p];
    SCHRO_HIP_REQUIRE (pl.coeffs && pl.quant && pl.summary && pl.codeblocks && pl.ncodeblocks > 0 && pl.bytes > 0
        && ((uintptr_t) pl.coeffs | (uintptr_t) pl.quant) % bpp == 0 && (uintptr_t) pl.summary % sizeof (uint32_t) == 0,
        "quantise_batch: plane %d invalid (coeffs, quant, summary, records and a size are needed, aligned to the sample)", p);
    const uintptr_t c0 = (uintptr_t) pl.coeffs, q0 = (uintptr_t) pl.quant;
    SCHRO_HIP_REQUIRE (c0 + pl.bytes <= q0 || q0 + pl.bytes <= c0, "quantise_batch: plane %d: quant overlaps coeffs", p);
    const int ndc = pl.dc_predict_first;
    SCHRO_HIP_REQUIRE (ndc >= 0 && ndc <= pl.ncodeblocks, "quantise_batch: plane %d: dc_predict_first %d of %d records", p, ndc,
        pl.ncodeblocks);
    if (ndc > 0)
      SCHRO_HIP_REQUIRE (pl.dc_width > 0 && pl.dc_height > 0 && pl.dc_height <= SCHRO_HIP_QUANTISE_DC_MAX_ROWS,
          "quantise_batch: plane %d: a DC band of %d x %d (1 .. %d rows)", p, pl.dc_width, pl.dc_height, SCHRO_HIP_QUANTISE_DC_MAX_ROWS);
    long long dc_area = 0;
    int dc_stride = 0;
    const size_t dc_rec_base = dc_recs.size (), job_base = jobs.size ();
    for (int c = 0; c < pl.ncodeblocks; c++) {
      const SchroHipCodeblock & cb = pl.codeblocks[c];
      SCHRO_HIP_REQUIRE (cb.width >= 0 && cb.height >= 0 && (allow_empty || (cb.width > 0 && cb.height > 0)),
          "quantise_batch: plane %d codeblock %d: %d x %d samples", p, c, cb.width, cb.height);
      if (cb.width == 0 || cb.height == 0)
        continue;
      if (chosen)
        SCHRO_HIP_REQUIRE (cb.quant_index < SCHRO_HIP_NOARITH_MAX_SUBBANDS,
            "quantise_chosen_batch: plane %d codeblock %d: quant_index %d is no sub-band (0 .. 18)", p, c, cb.quant_index);
      else
        SCHRO_HIP_REQUIRE (cb.quant_index <= 60, "quantise_batch: plane %d codeblock %d: quant_index %d", p, c, cb.quant_index);
      SCHRO_HIP_REQUIRE (cb.dst_stride > 0 && cb.dst_stride % bpp == 0 && (long long) cb.dst_stride >= (long long) cb.width * bpp,
          "quantise_batch: plane %d codeblock %d: a stride of %d bytes for rows of %d samples of %d bytes", p, c, cb.dst_stride,
          cb.width, bpp);
      SCHRO_HIP_REQUIRE (cb.dst_offset >= 0 && cb.dst_offset % bpp == 0
          && (unsigned long long) cb.dst_offset + (unsigned long long) (cb.height - 1) * cb.dst_stride
          + (unsigned long long) cb.width * bpp <= (unsigned long long) pl.bytes,
          "quantise_batch: plane %d codeblock %d (%d x %d at byte %d, pitch %d) reaches outside the plane's %zu bytes", p, c,
          cb.width, cb.height, cb.dst_offset, cb.dst_stride, pl.bytes);
      if (c < ndc) {
        if (!dc_stride)
          dc_stride = cb.dst_stride;
        SCHRO_HIP_REQUIRE (cb.dst_stride == dc_stride && (long long) pl.dc_width * bpp <= (long long) dc_stride,
            "quantise_batch: plane %d codeblock %d: the DC band's records share one stride, no shorter than the band's rows", p, c);
        QuantDcRec r;
        r.y0 = cb.dst_offset / cb.dst_stride;
        r.x0 = cb.dst_offset % cb.dst_stride / bpp;
        r.x1 = r.x0 + cb.width;
        r.y1 = r.y0 + cb.height;
        SCHRO_HIP_REQUIRE (r.x1 <= pl.dc_width && r.y1 <= pl.dc_height,
            "quantise_batch: plane %d codeblock %d (%d x %d at %d, %d) reaches outside the DC band of %d x %d", p, c, cb.width,
            cb.height, r.x0, r.y0, pl.dc_width, pl.dc_height);
        for (size_t k = dc_rec_base; k < dc_recs.size (); k++)
          SCHRO_HIP_REQUIRE (r.x0 >= dc_recs[k].x1 || r.x1 <= dc_recs[k].x0 || r.y0 >= dc_recs[k].y1 || r.y1 <= dc_recs[k].y0,
              "quantise_batch: plane %d codeblock %d overlaps codeblock %d of the DC band", p, c, dc_recs[k].index);
        QuantJob j;
        quant_job_constants (&j, cb.quant_index, pl.is_intra, 4);       // (C schro_quantise at both depths)
        r.factor = j.factor;
        r.offset = j.offset;
        r.index = c;
        r.pad = 0;
        if (chosen) {
          r.factor = r.offset = 0;
          r.pad = cb.quant_index;
        }
        dc_recs.push_back (r);
        dc_area += (long long) cb.width * cb.height;
        continue;
      }
      QuantJob j;
      memset (&j, 0, sizeof (j));
      j.coeffs = (char *) pl.coeffs + cb.dst_offset;
      j.quant = (char *) pl.quant + cb.dst_offset;
      j.summary = pl.summary + c;
      j.stride = cb.dst_stride;
      j.w = cb.width;
      j.h = cb.height;
      if (chosen)
        j.pad = cb.quant_index;
      else
        quant_job_constants (&j, cb.quant_index, pl.is_intra, bpp);
      j.tiles_x = div_up (cb.width, tw);
      total_tiles += (long long) j.tiles_x * div_up (cb.height, th);
      jobs.push_back (j);
    }
    if (chosen) {
      const QuantChosen jr = { chosen[p], (int) job_base, (int) (jobs.size () - job_base), pl.is_intra, 0 };
      const QuantChosen dr = { chosen[p], (int) dc_rec_base, (int) (dc_recs.size () - dc_rec_base), pl.is_intra, 0 };
      if (jr.count)
        job_runs.push_back (jr);
      if (dr.count)
        dc_runs.push_back (dr);
    }
    if (ndc > 0) {
      SCHRO_HIP_REQUIRE (dc_area == (long long) pl.dc_width * pl.dc_height,
          "quantise_batch: plane %d: the first %d records cover %lld of the DC band's %d x %d samples", p, ndc, dc_area,
          pl.dc_width, pl.dc_height);
      QuantDcJob d;
      memset (&d, 0, sizeof (d));
      d.coeffs = pl.coeffs;
      d.quant = pl.quant;
      d.summary = pl.summary;
      d.stride = dc_stride;
      d.w = pl.dc_width;
      d.h = pl.dc_height;
      d.rec_base = (int) dc_rec_base;
      d.nrec = (int) (dc_recs.size () - dc_rec_base);
      dc_jobs.push_back (d);
      dc_max_rows = std::max (dc_max_rows, pl.dc_height);
    }
  }

  SCHRO_HIP_REQUIRE (total_tiles < ((long long) 1 << 31), "quantise_batch: %lld tiles", total_tiles);

  for (int p = 0; p < nplanes; p++)
    SCHRO_HIP_CHECK (hipMemsetAsync (planes[p].summary, 0, sizeof (SchroHipCodeblockSummary) * (size_t) planes[p].ncodeblocks,
            ctx->stream));

  // one launch per 2^18 codeblocks (find_dequant_job's three probes), the table behind the jobs as dequant_batch builds it
  const size_t kPerLaunch = (size_t) 1 << 18;
  std::vector < char >table;
  const QuantChosen *d_job_runs = nullptr, *d_dc_runs = nullptr;
  if (chosen) {
    SCHRO_HIP_REQUIRE ((job_runs.size () + dc_runs.size ()) * sizeof (QuantChosen) <= SchroHipContext::kArgSlotBytes,
        "quantise_chosen_batch: %d planes are too many for one call", nplanes);
    std::vector < QuantChosen > runs (job_runs);
    runs.insert (runs.end (), dc_runs.begin (), dc_runs.end ());
    void *d_runs = nullptr;
    if (!runs.empty ()) {
      int r = push_args (ctx, runs.data (), runs.size () * sizeof (QuantChosen), &d_runs);
      if (r)
        return r;
    }
    d_job_runs = (const QuantChosen *) d_runs;
    d_dc_runs = d_job_runs + job_runs.size ();
  }
  for (size_t first = 0; first < jobs.size (); first += kPerLaunch) {
    const size_t n = std::min (kPerLaunch, jobs.size () - first), n64 = (n + 63) / 64, n4096 = (n + 4095) / 4096;
    long long tiles = 0;
    for (size_t k = 0; k < n; k++) {
      QuantJob & j = jobs[first + k];
      j.tile_base = (int) tiles;
      tiles += (long long) j.tiles_x * div_up (j.h, th);
    }
    const size_t bytes = sizeof (QuantJob) * n + sizeof (int) * (n + n64 + n4096);
    table.resize (bytes);
    memcpy (table.data (), jobs.data () + first, sizeof (QuantJob) * n);
    int *index = (int *) (table.data () + sizeof (QuantJob) * n);
    for (size_t k = 0; k < n; k++)
      index[k] = jobs[first + k].tile_base;
    for (size_t k = 0; k < n64; k++)
      index[n + k] = jobs[first + 64 * k].tile_base;
    for (size_t k = 0; k < n4096; k++)
      index[n + n64 + k] = jobs[first + 4096 * k].tile_base;
    void *d_jobs;
    int r = bytes <= SchroHipContext::kArgSlotBytes ? push_args (ctx, table.data (), bytes, &d_jobs)
        : push_big_table (ctx, table.data (), bytes, &d_jobs);
    if (r)
      return r;
    if (chosen) {
      r = launch_quantise_resolve (ctx->stream, (QuantJob *) d_jobs, (int) n, (int) first, d_job_runs, (int) job_runs.size (), bpp, clamped);
      if (r)
        return r;
    }
    ProfileScope ps (ctx, SCHRO_HIP_KERNEL_QUANTISE);
    r = launch_quantise (ctx->stream, (const QuantJob *) d_jobs, (int) n, (int) tiles, bpp);
    if (r)
      return r;
  }
  if (!dc_jobs.empty ()) {
    const size_t job_bytes = round_up (sizeof (QuantDcJob) * dc_jobs.size (), 16);
    const size_t bytes = job_bytes + sizeof (QuantDcRec) * dc_recs.size ();
    table.assign (bytes, 0);
    memcpy (table.data (), dc_jobs.data (), sizeof (QuantDcJob) * dc_jobs.size ());
    memcpy (table.data () + job_bytes, dc_recs.data (), sizeof (QuantDcRec) * dc_recs.size ());
    void *d_tab;
    int r = bytes <= SchroHipContext::kArgSlotBytes ? push_args (ctx, table.data (), bytes, &d_tab)
        : push_big_table (ctx, table.data (), bytes, &d_tab);
    if (r)
      return r;
    if (chosen) {
      r = launch_quantise_resolve_dc (ctx->stream, (QuantDcRec *) ((char *) d_tab + job_bytes), (int) dc_recs.size (), d_dc_runs,
          (int) dc_runs.size (), clamped);
      if (r)
        return r;
    }
    ProfileScope ps (ctx, SCHRO_HIP_KERNEL_QUANTISE_DC);
    return launch_quantise_dc (ctx->stream, (const QuantDcJob *) d_tab, (int) dc_jobs.size (),
        (const QuantDcRec *) ((const char *) d_tab + job_bytes), dc_max_rows, bpp);
  }
  return 0;
}

void
frame_quant_table_free (SchroHipContext * ctx)
{
  FrameQuantTable *t = ctx->frame_q_table;
  if (!t)
    return;
  if (t->d_summary) {
    for (int q = 0; q < SchroHipContext::kQueues; q++)  // launches that still write the summaries
      if (ctx->streams[q])
        (void) hipStreamSynchronize (ctx->streams[q]);
    (void) hipFree (t->d_summary);
  }
  delete t;
  ctx->frame_q_table = nullptr;
}

}                               // namespace schro

extern "C" {

int
schro_hip_quantise_batch (SchroHipContext * ctx, const SchroHipQuantPlane * planes, int nplanes, int bytes_per_sample)
{
  return quantise_batch_run (ctx, planes, nplanes, bytes_per_sample, false, nullptr, nullptr);
}

int
schro_hip_quantise_chosen_batch (SchroHipContext * ctx, const SchroHipQuantPlane * planes, const int32_t * const *chosen, int nplanes,
    int bytes_per_sample, uint32_t * clamped)
{
  SCHRO_HIP_REQUIRE (chosen, "quantise_chosen_batch: chosen is NULL");
  return quantise_batch_run (ctx, planes, nplanes, bytes_per_sample, false, chosen, clamped);
}

}                               // extern "C"
