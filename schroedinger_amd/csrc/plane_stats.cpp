// plane_stats.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: picture statistics -- the sums
// under the average luma and the squared error (schro_hip_plane_sums_batch), the recursive Gaussian low-pass
// (schro_hip_lowpass2_coeff, schro_hip_lowpass2_batch) and SSIM (schro_hip_ssim_batch), each with its host-only _check.

#include "schro_hip_internal.h"

#include <cmath>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr int kMaxStatsPlane = 1 << 16;
// SSIM: a picture's tiles are counted in an int, and its five low-pass planes share a table with the other pictures'
constexpr int kMaxSsimSize = 1 << 14, kMaxSsimPictures = 64;

struct SsimLayout {
  int stride8, stride16, tiles_x, ntiles;
  size_t a_low, b_low, ab, aa, bb, partial, bytes;
};

SsimLayout
ssim_layout (int w, int h)
{
  SsimLayout l;
  l.stride8 = (int) round_up ((size_t) w, 64);
  l.stride16 = (int) round_up ((size_t) w * 2, 64);
  l.tiles_x = div_up (w, kSsimTileCols);
  l.ntiles = l.tiles_x * div_up (h, kSsimTileRows);
  const size_t p8 = (size_t) l.stride8 * h, p16 = (size_t) l.stride16 * h;
  l.a_low = 0;
  l.b_low = p8;
  l.ab = 2 * p8;
  l.aa = l.ab + p16;
  l.bb = l.aa + p16;
  l.partial = l.bb + p16;
  l.bytes = l.partial + round_up ((size_t) l.ntiles * sizeof (double), 64);
  return l;
}

int
sums_build (const SchroHipSumsJob * jobs, int njobs, std::vector < SumsJob > &out, int *total_tiles)
{
  const char *who = "plane_sums_batch";
  SCHRO_HIP_REQUIRE (jobs && njobs > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (njobs <= kMaxJobs, "%s: at most %d jobs per call", who, kMaxJobs);
  out.resize (njobs);
  int tile_base = 0;
  for (int k = 0; k < njobs; k++) {
    const SchroHipSumsJob & s = jobs[k];
    SCHRO_HIP_REQUIRE (s.bytes_per_sample == 1 || s.bytes_per_sample == 2, "%s: job %d: %d bytes per sample is neither 1 nor 2", who, k,
        s.bytes_per_sample);
    SCHRO_HIP_REQUIRE (s.width > 0 && s.height > 0, "%s: job %d size %dx%d is not positive", who, k, s.width, s.height);
    SCHRO_HIP_REQUIRE (s.width <= kMaxStatsPlane && s.height <= kMaxStatsPlane, "%s: job %d size %dx%d is too large", who, k, s.width, s.height);
    SCHRO_HIP_REQUIRE (s.a && s.result, "%s: job %d has a NULL pointer", who, k);
    SCHRO_HIP_REQUIRE ((long long) s.a_stride >= (long long) s.width * s.bytes_per_sample, "%s: job %d: stride %d of a shorter than a row", who, k,
        s.a_stride);
    SCHRO_HIP_REQUIRE (s.bytes_per_sample == 1 || (((uintptr_t) s.a | (uintptr_t) s.a_stride) & 1) == 0,
        "%s: job %d: an s16 plane at an odd address or stride", who, k);
    SCHRO_HIP_REQUIRE (((uintptr_t) s.result & 7) == 0, "%s: job %d: the result is not 8-byte aligned", who, k);
    if (s.b) {
      SCHRO_HIP_REQUIRE (s.bytes_per_sample == 1, "%s: job %d: the squared error is of two u8 planes", who, k);
      SCHRO_HIP_REQUIRE (s.b_width == s.width && s.b_height == s.height, "%s: job %d: a is %dx%d, b is %dx%d", who, k, s.width, s.height,
          s.b_width, s.b_height);
      SCHRO_HIP_REQUIRE (s.b_stride >= s.width, "%s: job %d: stride %d of b shorter than a row", who, k, s.b_stride);
    }
    for (int m = 0; m < k; m++)
      SCHRO_HIP_REQUIRE (jobs[m].result + 2 <= s.result || s.result + 2 <= jobs[m].result, "%s: jobs %d and %d share a result", who, m, k);
    SumsJob & j = out[k];
    memset (&j, 0, sizeof (j));
    j.a = s.a;
    j.b = s.b;
    j.result = (unsigned long long *) s.result;
    j.a_stride = s.a_stride;
    j.b_stride = s.b_stride;
    j.w = s.width;
    j.h = s.height;
    j.bps = s.bytes_per_sample;
    j.tiles_x = div_up (s.width * s.bytes_per_sample, kSumsTileBytes);
    j.tile_base = tile_base;
    tile_base += j.tiles_x * div_up (s.height, kSumsTileRows);
  }
  *total_tiles = tile_base;
  return 0;
}

// A plane's bytes: `rows` runs of `row_bytes` bytes, `stride` apart (a span of bytes: one row).
struct Rect {
  uintptr_t begin;
  size_t stride, row_bytes, rows;
  uintptr_t end () const { return begin + stride * (rows - 1) + row_bytes; }
};

Rect
rect_of (const void *data, int stride, size_t row_bytes, int rows)
{
  return { (uintptr_t) data, (size_t) stride, row_bytes, (size_t) rows };
}

// Whether two planes share a byte.  Disjoint extents never do; planes of ONE stride whose extents meet -- windows of one
// buffer, side by side -- do not when their column ranges within the stride are apart; anything else whose extents meet
// counts as overlapping (no false "disjoint").
bool
rects_overlap (const Rect & a, const Rect & b)
{
  if (a.end () <= b.begin || b.end () <= a.begin)
    return false;
  if (a.stride != b.stride || a.rows < 2 || b.rows < 2)
    return true;
  const Rect & lo = a.begin <= b.begin ? a : b, &hi = a.begin <= b.begin ? b : a;
  const size_t d = (hi.begin - lo.begin) % lo.stride;   // hi's first column, counted from lo's
  return !(d >= lo.row_bytes && d + hi.row_bytes <= lo.stride);
}

bool
finite4 (const double *c)
{
  return std::isfinite (c[0]) && std::isfinite (c[1]) && std::isfinite (c[2]) && std::isfinite (c[3]);
}

int
lowpass_build (const char *who, const SchroHipLowpass2Plane * planes, int nplanes, std::vector < LowpassJob > &out, int *row_groups,
    int *col_groups)
{
  SCHRO_HIP_REQUIRE (planes && nplanes > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (nplanes <= kMaxJobs, "%s: at most %d planes per call", who, kMaxJobs);
  out.resize (nplanes);
  int rows = 0, cols = 0;
  for (int k = 0; k < nplanes; k++) {
    const SchroHipLowpass2Plane & p = planes[k];
    SCHRO_HIP_REQUIRE (p.bytes_per_sample == 1 || p.bytes_per_sample == 2, "%s: plane %d: %d bytes per sample is neither 1 nor 2", who, k,
        p.bytes_per_sample);
    SCHRO_HIP_REQUIRE (p.width > 0 && p.height > 0, "%s: plane %d size %dx%d is not positive", who, k, p.width, p.height);
    SCHRO_HIP_REQUIRE (p.width <= kMaxStatsPlane && p.height <= kMaxStatsPlane, "%s: plane %d size %dx%d is too large", who, k, p.width,
        p.height);
    SCHRO_HIP_REQUIRE (p.data && p.out_of_range, "%s: plane %d has a NULL pointer", who, k);
    SCHRO_HIP_REQUIRE ((long long) p.stride >= (long long) p.width * p.bytes_per_sample, "%s: plane %d: stride %d shorter than a row", who, k,
        p.stride);
    SCHRO_HIP_REQUIRE (p.bytes_per_sample == 1 || (((uintptr_t) p.data | (uintptr_t) p.stride) & 1) == 0,
        "%s: plane %d: an s16 plane at an odd address or stride", who, k);
    SCHRO_HIP_REQUIRE (((uintptr_t) p.out_of_range & 3) == 0, "%s: plane %d: the counter is not 4-byte aligned", who, k);
    SCHRO_HIP_REQUIRE (finite4 (p.h_coeff) && finite4 (p.v_coeff), "%s: plane %d has a coefficient that is not finite", who, k);
    for (int m = 0; m < k; m++)
      SCHRO_HIP_REQUIRE (!rects_overlap (rect_of (p.data, p.stride, p.width * p.bytes_per_sample, p.height),
              rect_of (planes[m].data, planes[m].stride, planes[m].width * planes[m].bytes_per_sample, planes[m].height)),
          "%s: planes %d and %d overlap", who, m, k);
    LowpassJob & j = out[k];
    memset (&j, 0, sizeof (j));
    j.data = p.data;
    j.out_of_range = p.out_of_range;
    memcpy (j.hc, p.h_coeff, sizeof (j.hc));
    memcpy (j.vc, p.v_coeff, sizeof (j.vc));
    j.stride = p.stride;
    j.w = p.width;
    j.h = p.height;
    j.bps = p.bytes_per_sample;
    j.row_base = rows;
    j.col_base = cols;
    rows += div_up (p.height, kLowpassRows);
    cols += div_up (p.width, kLowpassCols);
  }
  *row_groups = rows;
  *col_groups = cols;
  return 0;
}

int
lowpass_run (const char *who, SchroHipContext * ctx, const SchroHipLowpass2Plane * planes, int nplanes)
{
  std::vector < LowpassJob > jobs;
  int rows, cols;
  int r = lowpass_build (who, planes, nplanes, jobs, &rows, &cols);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);
  void *d_jobs;
  r = push_args (ctx, jobs.data (), sizeof (LowpassJob) * jobs.size (), &d_jobs);
  if (r)
    return r;
  return launch_lowpass2 (ctx->stream, (const LowpassJob *) d_jobs, nplanes, rows, cols);
}

// scratch, result, map (rows 0 without one), a, b of a picture whose own refusals have passed
void
ssim_rects (const SchroHipSsimPicture & p, Rect * r)
{
  r[0] = rect_of (p.scratch, 0, ssim_layout (p.width, p.height).bytes, 1);
  r[1] = rect_of (p.result, 0, sizeof (SchroHipSsimResult), 1);
  r[2] = rect_of (p.map, p.map_stride, (size_t) p.width * 8, p.map ? p.height : 0);
  r[3] = rect_of (p.a, p.a_stride, p.width, p.height);
  r[4] = rect_of (p.b, p.b_stride, p.width, p.height);
}

int
ssim_build (const SchroHipSsimPicture * pictures, int npictures, std::vector < SsimJob > &out, int *total_tiles)
{
  const char *who = "ssim_batch";
  SCHRO_HIP_REQUIRE (pictures && npictures > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (npictures <= kMaxSsimPictures, "%s: at most %d pictures per call", who, kMaxSsimPictures);
  out.resize (npictures);
  int tile_base = 0;
  for (int k = 0; k < npictures; k++) {
    const SchroHipSsimPicture & p = pictures[k];
    SCHRO_HIP_REQUIRE (p.width > 0 && p.height > 0, "%s: picture %d size %dx%d is not positive", who, k, p.width, p.height);
    SCHRO_HIP_REQUIRE (p.width <= kMaxSsimSize && p.height <= kMaxSsimSize, "%s: picture %d size %dx%d is too large", who, k, p.width, p.height);
    SCHRO_HIP_REQUIRE (p.a && p.b && p.scratch && p.result, "%s: picture %d has a NULL pointer", who, k);
    SCHRO_HIP_REQUIRE (p.b_width == p.width && p.b_height == p.height, "%s: picture %d: a is %dx%d, b is %dx%d", who, k, p.width, p.height,
        p.b_width, p.b_height);
    SCHRO_HIP_REQUIRE (p.a_stride >= p.width && p.b_stride >= p.width, "%s: picture %d: a stride shorter than a row", who, k);
    SCHRO_HIP_REQUIRE (((uintptr_t) p.result & 7) == 0, "%s: picture %d: the result is not 8-byte aligned", who, k);
    SCHRO_HIP_REQUIRE (((uintptr_t) p.scratch & 15) == 0, "%s: picture %d: the scratch is not 16-byte aligned", who, k);
    const SsimLayout l = ssim_layout (p.width, p.height);
    SCHRO_HIP_REQUIRE (p.scratch_bytes >= l.bytes, "%s: picture %d: %zu bytes of scratch, %zu needed", who, k, p.scratch_bytes, l.bytes);
    if (p.map) {
      SCHRO_HIP_REQUIRE (((uintptr_t) p.map & 7) == 0 && (p.map_stride & 7) == 0, "%s: picture %d: the map is not 8-byte aligned", who, k);
      SCHRO_HIP_REQUIRE ((long long) p.map_stride >= (long long) p.width * 8, "%s: picture %d: stride %d of the map shorter than a row", who, k,
          p.map_stride);
    }
    // what the picture writes -- its scratch, its result, its map -- shares no byte with anything the call reads or writes
    const char *const names[5] = { "scratch", "a result", "a map", "plane a", "plane b" };
    for (int m = 0; m <= k; m++) {
      Rect mine[5], theirs[5];
      ssim_rects (p, mine);
      ssim_rects (pictures[m], theirs);
      for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) {
          if ((i >= 3 && j >= 3) || (m == k && j <= i) || !mine[i].rows || !theirs[j].rows)
            continue;           // (two inputs may be one plane; a picture's own pairs once)
          if (i == j && m != k)
            SCHRO_HIP_REQUIRE (!rects_overlap (mine[i], theirs[j]), "%s: pictures %d and %d share %s", who, m, k, names[i]);
          else
            SCHRO_HIP_REQUIRE (!rects_overlap (mine[i], theirs[j]), "%s: %s of picture %d overlaps %s of picture %d", who,
                i < 3 ? names[i] : names[j], i < 3 ? k : m, i < 3 ? names[j] : names[i], i < 3 ? m : k);
        }
    }
    SsimJob & j = out[k];
    memset (&j, 0, sizeof (j));
    char *s = (char *) p.scratch;
    j.a = p.a;
    j.b = p.b;
    j.a_low = (uint8_t *) (s + l.a_low);
    j.b_low = (uint8_t *) (s + l.b_low);
    j.ab = (int16_t *) (s + l.ab);
    j.aa = (int16_t *) (s + l.aa);
    j.bb = (int16_t *) (s + l.bb);
    j.partial = (double *) (s + l.partial);
    j.result = p.result;
    j.map = p.map;
    j.a_stride = p.a_stride;
    j.b_stride = p.b_stride;
    j.stride8 = l.stride8;
    j.stride16 = l.stride16;
    j.map_stride = p.map_stride;
    j.w = p.width;
    j.h = p.height;
    j.tiles_x = l.tiles_x;
    j.ntiles = l.ntiles;
    j.tile_base = tile_base;
    tile_base += l.ntiles;
  }
  *total_tiles = tile_base;
  return 0;
}

}                               // namespace

extern "C" {

int
schro_hip_plane_sums_check (const SchroHipSumsJob * jobs, int njobs)
{
  std::vector < SumsJob > table;
  int tiles;
  return sums_build (jobs, njobs, table, &tiles);
}

int
schro_hip_plane_sums_batch (SchroHipContext * ctx, const SchroHipSumsJob * jobs, int njobs)
{
  SCHRO_HIP_REQUIRE (ctx, "plane_sums_batch: no context");
  std::vector < SumsJob > table;
  int tiles;
  int r = sums_build (jobs, njobs, table, &tiles);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);
  void *d_jobs;
  r = push_args (ctx, table.data (), sizeof (SumsJob) * table.size (), &d_jobs);
  if (r)
    return r;
  return launch_plane_sums (ctx->stream, (const SumsJob *) d_jobs, njobs, tiles);
}

// generate_coeff (schrofilter.c:666-689), statement by statement
void
schro_hip_lowpass2_coeff (double sigma, double coeff[4])
{
  double q;
  if (sigma >= 2.5)
    q = 0.98711 * sigma - 0.96330;
  else
    q = 3.97156 - 4.41554 * sqrt (1 - 0.26891 * sigma);
  const double b0 = 1.57825 + 2.44413 * q + 1.4281 * q * q + 0.422205 * q * q * q;
  const double b0inv = 1.0 / b0;
  const double b1 = 2.44413 * q + 2.85619 * q * q + 1.26661 * q * q * q;
  const double b2 = -1.4281 * q * q - 1.26661 * q * q * q;
  const double b3 = 0.422205 * q * q * q;
  const double B = 1 - (b1 + b2 + b3) / b0;
  coeff[0] = B;
  coeff[1] = b1 * b0inv;
  coeff[2] = b2 * b0inv;
  coeff[3] = b3 * b0inv;
}

int
schro_hip_lowpass2_check (const SchroHipLowpass2Plane * planes, int nplanes)
{
  std::vector < LowpassJob > table;
  int rows, cols;
  return lowpass_build ("lowpass2_batch", planes, nplanes, table, &rows, &cols);
}

int
schro_hip_lowpass2_batch (SchroHipContext * ctx, const SchroHipLowpass2Plane * planes, int nplanes)
{
  SCHRO_HIP_REQUIRE (ctx, "lowpass2_batch: no context");
  return lowpass_run ("lowpass2_batch", ctx, planes, nplanes);
}

size_t
schro_hip_ssim_scratch_bytes (int width, int height)
{
  if (width <= 0 || height <= 0 || width > kMaxSsimSize || height > kMaxSsimSize)
    return 0;
  return ssim_layout (width, height).bytes;
}

void
schro_hip_picture_stats_geometry (int values[SCHRO_HIP_PICTURE_STATS_GEOMETRY])
{
  const int v[SCHRO_HIP_PICTURE_STATS_GEOMETRY] = { kSumsTileBytes, kSumsTileRows, kLowpassRows, kLowpassChunk, kLowpassCols, kLowpassColRows,
    kSsimTileCols, kSsimTileRows
  };
  memcpy (values, v, sizeof (v));
}

int
schro_hip_ssim_check (const SchroHipSsimPicture * pictures, int npictures)
{
  std::vector < SsimJob > table;
  int tiles;
  return ssim_build (pictures, npictures, table, &tiles);
}

int
schro_hip_ssim_batch (SchroHipContext * ctx, const SchroHipSsimPicture * pictures, int npictures)
{
  SCHRO_HIP_REQUIRE (ctx, "ssim_batch: no context");
  std::vector < SsimJob > table;
  int tiles;
  int r = ssim_build (pictures, npictures, table, &tiles);
  if (r)
    return r;
  // the low-passes: a_lowpass, b_lowpass as u8 in one launch pair; then ab, a^2, b^2 as s16 in another
  std::vector < SchroHipLowpass2Plane > low8 (2 * (size_t) npictures), low16 (3 * (size_t) npictures);
  for (int k = 0; k < npictures; k++) {
    const SsimJob & j = table[k];
    double coeff[4];
    schro_hip_lowpass2_coeff (j.w / 256.0 * 1.5, coeff);
    SCHRO_HIP_REQUIRE (finite4 (coeff), "ssim_batch: picture %d: no coefficients for width %d", k, j.w);
    void *const data[5] = { j.a_low, j.b_low, j.ab, j.aa, j.bb };
    for (int m = 0; m < 5; m++) {
      SchroHipLowpass2Plane & p = m < 2 ? low8[2 * (size_t) k + m] : low16[3 * (size_t) k + m - 2];
      memset (&p, 0, sizeof (p));
      p.data = data[m];
      p.bytes_per_sample = m < 2 ? 1 : 2;
      p.stride = m < 2 ? j.stride8 : j.stride16;
      p.width = j.w;
      p.height = j.h;
      memcpy (p.h_coeff, coeff, sizeof (coeff));
      memcpy (p.v_coeff, coeff, sizeof (coeff));
      p.out_of_range = &j.result->out_of_range[m];
    }
  }
  (void) hipSetDevice (ctx->device);
  void *d_jobs;
  r = push_args (ctx, table.data (), sizeof (SsimJob) * table.size (), &d_jobs);
  if (r)
    return r;
  const SsimJob *d = (const SsimJob *) d_jobs;
  if ((r = launch_ssim_prepare (ctx->stream, d, npictures, tiles)))
    return r;
  if ((r = lowpass_run ("ssim_batch", ctx, low8.data (), (int) low8.size ())))
    return r;
  if ((r = launch_ssim_products (ctx->stream, d, npictures, tiles)))
    return r;
  if ((r = lowpass_run ("ssim_batch", ctx, low16.data (), (int) low16.size ())))
    return r;
  return launch_ssim_final (ctx->stream, d, npictures, tiles);
}

}                               // extern "C"
