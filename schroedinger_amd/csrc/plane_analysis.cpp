// plane_analysis.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: encoder analysis -- the
// downsample pyramid (schro_hip_downsample_batch), the SAD scan (schro_hip_metric_scan_setup, schro_hip_metric_scan_batch)
// and the loop of schro_rough_me_heirarchical_scan_nohint over it (rough_scan_nohint_run, the frame layer's call).

#include "schro_hip_internal.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

// SchroMotionVector (schromotion.h:20-37)
struct MotionVector {
  uint32_t flags;               // pred_mode : 2, using_global : 1, split : 2, unused : 3, scan : 8
  uint32_t metric;
  uint32_t chroma_metric;
  int16_t dx[2];
  int16_t dy[2];
};
static_assert (sizeof (MotionVector) == 20, "SchroMotionVector");

constexpr int kMaxPlaneSize = 1 << 16;
constexpr int kMaxExtension = 1024;

}                               // namespace

namespace schro {

int
rough_scan_nohint_run (SchroHipContext * ctx, const uint8_t * frame, int frame_stride, const uint8_t * ref, int ref_stride,
    int width, int height, int extension, const SchroHipParams * params, int shift, int distance, int ref_index,
    void *motion_vectors)
{
  SCHRO_HIP_REQUIRE (ctx && frame && ref && params && motion_vectors, "rough_scan_nohint: bad arguments");
  SCHRO_HIP_REQUIRE (params->x_num_blocks > 0 && params->y_num_blocks > 0 && params->x_num_blocks <= (1 << 14)
      && params->y_num_blocks <= (1 << 14), "rough_scan_nohint: %d x %d blocks", params->x_num_blocks, params->y_num_blocks);
  SCHRO_HIP_REQUIRE (params->xbsep_luma > 0 && params->ybsep_luma > 0 && params->xbsep_luma <= SCHRO_HIP_LIMIT_BLOCK_SIZE
      && params->ybsep_luma <= SCHRO_HIP_LIMIT_BLOCK_SIZE, "rough_scan_nohint: block separation %d x %d out of range",
      params->xbsep_luma, params->ybsep_luma);
  SCHRO_HIP_REQUIRE (shift >= 0 && shift <= 8, "rough_scan_nohint: shift %d out of range", shift);
  SCHRO_HIP_REQUIRE (distance > 0, "rough_scan_nohint: distance %d", distance);
  SCHRO_HIP_REQUIRE (ref_index == 0 || ref_index == 1, "rough_scan_nohint: reference %d is neither 0 nor 1", ref_index);
  SCHRO_HIP_REQUIRE (width > 0 && height > 0 && width <= kMaxPlaneSize && height <= kMaxPlaneSize && extension >= 0
      && extension <= kMaxExtension, "rough_scan_nohint: picture %d x %d, extension %d", width, height, extension);

  const int nbx = params->x_num_blocks, nby = params->y_num_blocks;
  MotionVector *mvs = (MotionVector *) motion_vectors;
  // schro_motion_field_set (mf, 0, 1)
  for (size_t n = 0; n < (size_t) nbx * nby; n++) {
    memset (&mvs[n], 0, sizeof (MotionVector));
    mvs[n].flags = 1;
  }
  std::vector < SchroHipMetricScan > scans;
  std::vector < size_t > where;
  const int skip = 1 << shift;
  for (int j = 0; j < nby; j += skip)
    for (int i = 0; i < nbx; i += skip) {
      SchroHipMetricScan s;
      memset (&s, 0, sizeof (s));
      s.x = (i >> shift) * params->xbsep_luma;
      s.y = (j >> shift) * params->ybsep_luma;
      s.block_width = std::min (width - s.x, params->xbsep_luma);
      s.block_height = std::min (height - s.y, params->ybsep_luma);
      int r = schro_hip_metric_scan_setup (&s, width, height, extension, 0, 0, distance);
      if (r)
        return r;
      s.dx = s.gravity_x = s.ref_x - s.x;
      s.dy = s.gravity_y = s.ref_y - s.y;
      MotionVector & mv = mvs[(size_t) j * nbx + i];
      if (s.scan_width <= 0 || s.scan_height <= 0) {
        mv.dx[0] = mv.dy[0] = 0;
        mv.metric = INT_MAX;    // SCHRO_METRIC_INVALID
        continue;
      }
      scans.push_back (s);
      where.push_back ((size_t) j * nbx + i);
    }
  if (scans.empty ())
    return 0;

  (void) hipSetDevice (ctx->device);
  const size_t bytes = scans.size () * sizeof (SchroHipMetricScanResult);
  int r = ensure_scratch (ctx, bytes);
  if (r)
    return r;
  SchroHipMetricScanPicture pic;
  memset (&pic, 0, sizeof (pic));
  pic.frame = frame;
  pic.frame_stride = frame_stride;
  pic.ref = ref;
  pic.ref_stride = ref_stride;
  pic.width = width;
  pic.height = height;
  pic.extension = extension;
  pic.scans = scans.data ();
  pic.nscans = (int) scans.size ();
  pic.results = (SchroHipMetricScanResult *) ctx->scratch_ref ();
  r = schro_hip_metric_scan_batch (ctx, &pic, 1);
  if (r)
    return r;
  std::vector < SchroHipMetricScanResult > results (scans.size ());
  SCHRO_HIP_CHECK (hipMemcpyAsync (results.data (), pic.results, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  for (size_t n = 0; n < scans.size (); n++) {
    MotionVector & mv = mvs[where[n]];
    mv.metric = results[n].metric;
    // dx <<= shift into the int16 member (unsigned: the vectors are negative as often as not)
    mv.dx[ref_index] = (int16_t) (uint16_t) ((uint32_t) results[n].dx << shift);
    mv.dy[ref_index] = (int16_t) (uint16_t) ((uint32_t) results[n].dy << shift);
  }
  return 0;
}

}                               // namespace schro

extern "C" {

int
schro_hip_downsample_batch (SchroHipContext * ctx, const SchroHipDownsamplePlane * planes, int nplanes)
{
  SCHRO_HIP_REQUIRE (ctx && planes && nplanes > 0, "downsample_batch: bad arguments");
  SCHRO_HIP_REQUIRE (nplanes <= kMaxJobs, "downsample_batch: at most %d planes per call", kMaxJobs);
  int tc, tr;
  downsample_tile_geometry (&tc, &tr);
  std::vector < DownsampleJob > jobs (nplanes);
  int tile_base = 0;
  for (int p = 0; p < nplanes; p++) {
    const SchroHipDownsamplePlane & pl = planes[p];
    SCHRO_HIP_REQUIRE (pl.src && pl.dst, "downsample_batch: plane %d has a NULL pointer", p);
    SCHRO_HIP_REQUIRE (pl.src_width > 0 && pl.src_height > 0, "downsample_batch: plane %d size %dx%d is not positive", p, pl.src_width,
        pl.src_height);
    SCHRO_HIP_REQUIRE (pl.src_width <= kMaxPlaneSize && pl.src_height <= kMaxPlaneSize, "downsample_batch: plane %d size %dx%d is too large",
        p, pl.src_width, pl.src_height);
    SCHRO_HIP_REQUIRE (pl.dst_extension >= 0, "downsample_batch: plane %d has a negative extension %d", p, pl.dst_extension);
    SCHRO_HIP_REQUIRE (pl.dst_extension <= kMaxExtension, "downsample_batch: plane %d extension %d is too large", p, pl.dst_extension);
    const int dw = (pl.src_width + 1) / 2, dh = (pl.src_height + 1) / 2, ext = pl.dst_extension;
    SCHRO_HIP_REQUIRE (pl.src_stride >= pl.src_width, "downsample_batch: plane %d src stride %d shorter than a row", p, pl.src_stride);
    SCHRO_HIP_REQUIRE (pl.dst_stride >= dw + 2 * ext, "downsample_batch: plane %d dst stride %d shorter than a row plus its aprons (%d)", p,
        pl.dst_stride, dw + 2 * ext);
    const uintptr_t s0 = (uintptr_t) pl.src, s1 = s0 + (size_t) pl.src_stride * (pl.src_height - 1) + pl.src_width;
    const uintptr_t d0 = (uintptr_t) pl.dst - (size_t) pl.dst_stride * ext - ext;
    const uintptr_t d1 = (uintptr_t) pl.dst + (size_t) pl.dst_stride * (dh + ext - 1) + dw + ext;
    SCHRO_HIP_REQUIRE (s1 <= d0 || d1 <= s0, "downsample_batch: plane %d src and dst overlap", p);

    DownsampleJob & j = jobs[p];
    memset (&j, 0, sizeof (j));
    j.src = pl.src;
    j.dst = pl.dst;
    j.src_stride = pl.src_stride;
    j.dst_stride = pl.dst_stride;
    j.sw = pl.src_width;
    j.sh = pl.src_height;
    j.dw = dw;
    j.dh = dh;
    j.ext = ext;
    // the groups of four start where a row's stores are dword-aligned (when the stride keeps that from row to row)
    j.xorg = -ext - (int) (((uintptr_t) pl.dst - ext) & 3);
    j.tiles_x = div_up (dw + ext - j.xorg, tc);
    j.m_tiles_x = div_magic (j.tiles_x);
    j.tile_base = tile_base;
    tile_base += j.tiles_x * div_up (dh + 2 * ext, tr);
  }
  (void) hipSetDevice (ctx->device);
  void *d_jobs;
  int r = push_args (ctx, jobs.data (), sizeof (DownsampleJob) * jobs.size (), &d_jobs);
  if (r)
    return r;
  return launch_downsample (ctx->stream, (const DownsampleJob *) d_jobs, nplanes, tile_base);
}

int
schro_hip_metric_scan_setup (SchroHipMetricScan * scan, int frame_width, int frame_height, int extension, int dx, int dy, int dist)
{
  SCHRO_HIP_REQUIRE (scan && dist > 0, "metric_scan_setup: needs a scan and a distance > 0");
  int xmin = std::max (-scan->block_width, scan->x + dx - dist);
  int xmax = std::min (frame_width, scan->x + dx + dist);
  int ymin = std::max (-scan->block_height, scan->y + dy - dist);
  int ymax = std::min (frame_height, scan->y + dy + dist);
  xmin = std::max (xmin, -extension);
  ymin = std::max (ymin, -extension);
  xmax = std::min (xmax, frame_width - scan->block_width + extension);
  ymax = std::min (ymax, frame_height - scan->block_height + extension);
  scan->ref_x = xmin;
  scan->ref_y = ymin;
  scan->scan_width = xmax - xmin + 1;
  scan->scan_height = ymax - ymin + 1;
  SCHRO_HIP_REQUIRE (scan->scan_width <= SCHRO_HIP_LIMIT_METRIC_SCAN && scan->scan_height <= SCHRO_HIP_LIMIT_METRIC_SCAN,
      "metric_scan_setup: a window of %d x %d positions is over the limit of %d", scan->scan_width, scan->scan_height,
      SCHRO_HIP_LIMIT_METRIC_SCAN);
  return 0;
}

int
schro_hip_metric_scan_batch (SchroHipContext * ctx, const SchroHipMetricScanPicture * pictures, int npictures)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && npictures > 0, "metric_scan_batch: bad arguments");
  SCHRO_HIP_REQUIRE (npictures <= kMaxJobs, "metric_scan_batch: at most %d pictures per call", kMaxJobs);
  size_t total = 0, lds = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipMetricScanPicture & pic = pictures[p];
    SCHRO_HIP_REQUIRE (pic.frame && pic.ref && pic.scans && pic.results, "metric_scan_batch: picture %d has a NULL pointer", p);
    SCHRO_HIP_REQUIRE (pic.width > 0 && pic.height > 0 && pic.width <= kMaxPlaneSize && pic.height <= kMaxPlaneSize,
        "metric_scan_batch: picture %d size %dx%d out of range", p, pic.width, pic.height);
    SCHRO_HIP_REQUIRE (pic.frame_stride >= pic.width && pic.ref_stride >= pic.width, "metric_scan_batch: picture %d: a stride shorter than a row", p);
    SCHRO_HIP_REQUIRE (pic.extension >= 0 && pic.extension <= kMaxExtension, "metric_scan_batch: picture %d extension %d out of range", p,
        pic.extension);
    SCHRO_HIP_REQUIRE (pic.nscans > 0 && pic.nscans <= (1 << 24), "metric_scan_batch: picture %d has %d scans", p, pic.nscans);
    for (int k = 0; k < pic.nscans; k++) {
      const SchroHipMetricScan & s = pic.scans[k];
      SCHRO_HIP_REQUIRE (s.scan_width > 0 && s.scan_height > 0, "metric_scan_batch: picture %d scan %d: a window of %d x %d positions", p, k,
          s.scan_width, s.scan_height);
      SCHRO_HIP_REQUIRE (s.scan_width <= SCHRO_HIP_LIMIT_METRIC_SCAN && s.scan_height <= SCHRO_HIP_LIMIT_METRIC_SCAN,
          "metric_scan_batch: picture %d scan %d: a window of %d x %d positions is over the limit of %d", p, k, s.scan_width, s.scan_height,
          SCHRO_HIP_LIMIT_METRIC_SCAN);
      SCHRO_HIP_REQUIRE (s.block_width <= SCHRO_HIP_LIMIT_BLOCK_SIZE && s.block_height <= SCHRO_HIP_LIMIT_BLOCK_SIZE,
          "metric_scan_batch: picture %d scan %d: a block of %d x %d is over %d x %d", p, k, s.block_width, s.block_height,
          SCHRO_HIP_LIMIT_BLOCK_SIZE, SCHRO_HIP_LIMIT_BLOCK_SIZE);
      // schrometric.c:38-45 (64-bit: the members are the caller's)
      SCHRO_HIP_REQUIRE ((long long) s.ref_x >= -pic.extension && (long long) s.ref_y >= -pic.extension,
          "metric_scan_batch: picture %d scan %d: the window starts at %d, %d, in front of the apron of %d", p, k, s.ref_x, s.ref_y,
          pic.extension);
      SCHRO_HIP_REQUIRE ((long long) s.ref_x + s.block_width + s.scan_width - 1 <= (long long) pic.width + pic.extension
          && (long long) s.ref_y + s.block_height + s.scan_height - 1 <= (long long) pic.height + pic.extension,
          "metric_scan_batch: picture %d scan %d: the window ends behind the apron of %d", p, k, pic.extension);
      const long long gi = (long long) s.gravity_x + s.x - s.ref_x, gj = (long long) s.gravity_y + s.y - s.ref_y;
      SCHRO_HIP_REQUIRE (gi >= 0 && gi < s.scan_width && gj >= 0 && gj < s.scan_height,
          "metric_scan_batch: picture %d scan %d: the gravity position %lld, %lld is outside the window", p, k, gi, gj);
      SCHRO_HIP_REQUIRE (s.x > -(1 << 20) && s.x < (1 << 20) && s.y > -(1 << 20) && s.y < (1 << 20) && s.block_width > -(1 << 20)
          && s.block_height > -(1 << 20), "metric_scan_batch: picture %d scan %d: block position out of range", p, k);
      lds = std::max (lds, scan_lds_bytes (s.block_width, s.block_height, s.scan_width, s.scan_height));
    }
    total += (size_t) pic.nscans;
  }
  SCHRO_HIP_REQUIRE (total <= (size_t) 1 << 26, "metric_scan_batch: %zu scans in one call", total);
  SCHRO_HIP_REQUIRE (lds <= scan_lds_limit (), "metric_scan_batch: a scan needs %zu bytes of LDS", lds);

  (void) hipSetDevice (ctx->device);
  const size_t head = sizeof (ScanPicture) * (size_t) npictures, bytes = head + sizeof (ScanJob) * total;
  void *host, *dev;
  int r = big_table_begin (ctx, bytes, &host, &dev);
  if (r)
    return r;
  ScanPicture *hp = (ScanPicture *) host;
  ScanJob *hs = (ScanJob *) ((char *) host + head);
  size_t base = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipMetricScanPicture & pic = pictures[p];
    ScanPicture & d = hp[p];
    memset (&d, 0, sizeof (d));
    d.frame = pic.frame;
    d.ref = pic.ref;
    d.results = pic.results;
    d.metrics = pic.metrics;
    d.frame_stride = pic.frame_stride;
    d.ref_stride = pic.ref_stride;
    d.width = pic.width;
    d.height = pic.height;
    d.scan_base = (int) base;
    for (int k = 0; k < pic.nscans; k++) {
      const SchroHipMetricScan & s = pic.scans[k];
      ScanJob & j = hs[base + k];
      memset (&j, 0, sizeof (j));
      j.x = s.x;
      j.y = s.y;
      j.bw = s.block_width;
      j.bh = s.block_height;
      j.ref_x = s.ref_x;
      j.ref_y = s.ref_y;
      j.sw = s.scan_width;
      j.sh = s.scan_height;
      j.gi = s.gravity_x + s.x - s.ref_x;
      j.gj = s.gravity_y + s.y - s.ref_y;
      j.dx = s.dx;
      j.dy = s.dy;
      j.pic = p;
      j.m_sh = div_magic (s.scan_height);
    }
    base += (size_t) pic.nscans;
  }
  r = big_table_commit (ctx, bytes);
  if (r)
    return r;
  return launch_metric_scan (ctx->stream, (const ScanPicture *) dev, (const ScanJob *) ((const char *) dev + head), (int) total, lds);
}

}                               // extern "C"
