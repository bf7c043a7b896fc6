// picture_stats_walk.cpp -- the host code of the picture statistics (plane_stats.cpp and the frame layer's five calls)
// walked under AddressSanitizer + UndefinedBehaviorSanitizer: a plain C++ program with its own main, linked with the
// objects of the library's device-free sanitizer build (make -C schroedinger_amd/csrc dry_asan).  Launches are dropped
// there, so what runs is every refusal, the job tables, the scratch layout and the sizing of the queue's scratch -- each
// batch call in a small, larger, small order -- and the frame layer's calls on frames of the "device" domain.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "picture_stats_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

static char *block;
static const size_t kBlock = (size_t) 192 << 20;
static int refusals = 0;

static size_t
take (size_t & off, size_t bytes, size_t align)
{
  off = (off + align - 1) / align * align;
  const size_t at = off;
  off += bytes;
  if (off > kBlock) {
    fprintf (stderr, "picture_stats_walk: the block is too small\n");
    exit (2);
  }
  return at;
}

static SchroHipSumsJob
sums_job (size_t & off, int w, int h, int bps, bool with_b)
{
  SchroHipSumsJob j;
  memset (&j, 0, sizeof (j));
  j.a_stride = (w * bps + 15) / 16 * 16;
  j.a = block + take (off, (size_t) j.a_stride * h, 64);
  j.bytes_per_sample = bps;
  j.width = w;
  j.height = h;
  if (with_b) {
    j.b_stride = w;
    j.b = (const uint8_t *) block + take (off, (size_t) w * h, 1);
    j.b_width = w;
    j.b_height = h;
  }
  j.result = (int64_t *) (block + take (off, 16, 8));
  return j;
}

static SchroHipLowpass2Plane
lowpass_plane (size_t & off, int w, int h, int bps, double hs, double vs)
{
  SchroHipLowpass2Plane p;
  memset (&p, 0, sizeof (p));
  p.stride = (w * bps + 15) / 16 * 16;
  p.data = block + take (off, (size_t) p.stride * h, 64);
  p.bytes_per_sample = bps;
  p.width = w;
  p.height = h;
  schro_hip_lowpass2_coeff (hs, p.h_coeff);
  schro_hip_lowpass2_coeff (vs, p.v_coeff);
  p.out_of_range = (uint32_t *) (block + take (off, 4, 4));
  return p;
}

static SchroHipSsimPicture
ssim_picture (size_t & off, int w, int h, bool with_map)
{
  SchroHipSsimPicture p;
  memset (&p, 0, sizeof (p));
  p.a_stride = w + 3;
  p.a = (const uint8_t *) block + take (off, (size_t) p.a_stride * h, 1);
  p.b_stride = (w + 63) / 64 * 64;
  p.b = (const uint8_t *) block + take (off, (size_t) p.b_stride * h, 64);
  p.width = p.b_width = w;
  p.height = p.b_height = h;
  p.scratch_bytes = schro_hip_ssim_scratch_bytes (w, h);
  p.scratch = block + take (off, p.scratch_bytes, 16);
  p.result = (SchroHipSsimResult *) (block + take (off, sizeof (SchroHipSsimResult), 8));
  if (with_map) {
    p.map_stride = 8 * w + 8;
    p.map = (double *) (block + take (off, (size_t) p.map_stride * h, 8));
  }
  return p;
}

template < typename T, typename Call > static void
refuse (const char *what, const T & good, T bad, Call call, const char *says)
{
  // a good entry in front: the refusal names entry 1
  T two[2] = { good, bad };
  EXPECT (call (two, 2) == SCHRO_HIP_EINVAL, "%s is not refused", what);
  EXPECT (strstr (schro_hip_last_error (), says), "%s: the refusal does not say \"%s\"", what, says);
  EXPECT (strstr (schro_hip_last_error (), " 1"), "%s: the refusal does not name entry 1", what);
  refusals++;
}

int
main ()
{
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "picture_stats_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
    return 2;
  }
  block = (char *) schro_hip_domain_alloc (ctx, kBlock);
  if (!block) {
    fprintf (stderr, "picture_stats_walk: no memory: %s\n", schro_hip_last_error ());
    return 2;
  }
  memset (block, 0, kBlock);
  int calls = 0;

  // ---- the coefficients ------------------------------------------------------------------------------------------------
  const double sigmas[6] = { 0.375, 0.75, 1.5, 2.5, 5, 22.5 };
  for (double sigma : sigmas) {
    double c[4];
    schro_hip_lowpass2_coeff (sigma, c);
    EXPECT (std::isfinite (c[0]) && fabs (c[0] + c[1] + c[2] + c[3] - 1.0) < 1e-15, "sigma %g: the coefficients sum to %.17g", sigma,
        c[0] + c[1] + c[2] + c[3]);
  }

  // ---- refusals: through the _check twin AND the batch call, which launches nothing ------------------------------------
  {
    size_t off = 0;
    const SchroHipSumsJob good = sums_job (off, 48, 8, 1, true), other = sums_job (off, 48, 8, 1, true);
    auto both = [&](SchroHipSumsJob * j, int n) {
      const int r = schro_hip_plane_sums_check (j, n);
      EXPECT (schro_hip_plane_sums_batch (ctx, j, n) == r, "plane_sums: the check and the batch call differ");
      return r;
    };
    EXPECT (both (const_cast < SchroHipSumsJob * >(&good), 1) == 0, "the good sums job is refused");
    SchroHipSumsJob b;
    b = other, b.width = b.b_width = 0, refuse ("sums: no width", good, b, both, "not positive");
    b = other, b.height = b.b_height = -3, refuse ("sums: a negative height", good, b, both, "not positive");
    b = other, b.a_stride = 47, refuse ("sums: a short stride of a", good, b, both, "shorter than a row");
    b = other, b.b_stride = 47, refuse ("sums: a short stride of b", good, b, both, "shorter than a row");
    b = other, b.a = nullptr, refuse ("sums: a NULL plane", good, b, both, "NULL");
    b = other, b.result = nullptr, refuse ("sums: a NULL result", good, b, both, "NULL");
    b = other, b.result = (int64_t *) ((char *) other.result + 4), refuse ("sums: a misaligned result", good, b, both, "8-byte aligned");
    b = other, b.bytes_per_sample = 4, refuse ("sums: 4 bytes per sample", good, b, both, "neither 1 nor 2");
    b = other, b.b_width = 47, refuse ("sums: b narrower than a", good, b, both, "b is 47x8");
    b = other, b.b_height = 9, refuse ("sums: b taller than a", good, b, both, "b is 48x9");
    b = other, b.result = good.result, refuse ("sums: a shared result", good, b, both, "share a result");
    EXPECT (schro_hip_plane_sums_check (nullptr, 1) == SCHRO_HIP_EINVAL && schro_hip_plane_sums_check (&good, 0) == SCHRO_HIP_EINVAL,
        "sums: an empty call passes");
    EXPECT (schro_hip_plane_sums_batch (nullptr, &good, 1) == SCHRO_HIP_EINVAL, "sums: no context passes");
  }
  {
    size_t off = 0;
    const SchroHipLowpass2Plane good = lowpass_plane (off, 48, 8, 2, 1.5, 0.75), other = lowpass_plane (off, 48, 8, 2, 5, 0.375);
    auto both = [&](SchroHipLowpass2Plane * p, int n) {
      const int r = schro_hip_lowpass2_check (p, n);
      EXPECT (schro_hip_lowpass2_batch (ctx, p, n) == r, "lowpass2: the check and the batch call differ");
      return r;
    };
    EXPECT (both (const_cast < SchroHipLowpass2Plane * >(&good), 1) == 0, "the good low-pass plane is refused");
    SchroHipLowpass2Plane b;
    b = other, b.width = 0, refuse ("lowpass2: no width", good, b, both, "not positive");
    b = other, b.height = 0, refuse ("lowpass2: no height", good, b, both, "not positive");
    b = other, b.stride = 94, refuse ("lowpass2: a short stride", good, b, both, "shorter than a row");
    b = other, b.data = nullptr, refuse ("lowpass2: a NULL plane", good, b, both, "NULL");
    b = other, b.out_of_range = nullptr, refuse ("lowpass2: a NULL counter", good, b, both, "NULL");
    b = other, b.out_of_range = (uint32_t *) ((char *) other.out_of_range + 2), refuse ("lowpass2: a misaligned counter", good, b, both,
        "4-byte aligned");
    b = other, b.bytes_per_sample = 3, refuse ("lowpass2: 3 bytes per sample", good, b, both, "neither 1 nor 2");
    b = other, b.h_coeff[1] = NAN, refuse ("lowpass2: a NaN coefficient", good, b, both, "not finite");
    b = other, b.v_coeff[3] = INFINITY, refuse ("lowpass2: an infinite coefficient", good, b, both, "not finite");
    b = other, b.data = (char *) good.data + 2, refuse ("lowpass2: overlapping planes", good, b, both, "overlap");
    EXPECT (schro_hip_lowpass2_check (nullptr, 1) == SCHRO_HIP_EINVAL && schro_hip_lowpass2_check (&good, 0) == SCHRO_HIP_EINVAL,
        "lowpass2: an empty call passes");
    EXPECT (schro_hip_lowpass2_batch (nullptr, &good, 1) == SCHRO_HIP_EINVAL, "lowpass2: no context passes");
  }
  {
    size_t off = 0;
    const SchroHipSsimPicture good = ssim_picture (off, 48, 8, true), other = ssim_picture (off, 48, 8, true);
    auto both = [&](SchroHipSsimPicture * p, int n) {
      const int r = schro_hip_ssim_check (p, n);
      EXPECT (schro_hip_ssim_batch (ctx, p, n) == r, "ssim: the check and the batch call differ");
      return r;
    };
    EXPECT (both (const_cast < SchroHipSsimPicture * >(&good), 1) == 0, "the good ssim picture is refused");
    SchroHipSsimPicture b;
    b = other, b.width = b.b_width = 0, refuse ("ssim: no width", good, b, both, "not positive");
    b = other, b.height = b.b_height = 0, refuse ("ssim: no height", good, b, both, "not positive");
    b = other, b.a_stride = 47, refuse ("ssim: a short stride", good, b, both, "shorter than a row");
    b = other, b.b = nullptr, refuse ("ssim: a NULL plane", good, b, both, "NULL");
    b = other, b.scratch = nullptr, refuse ("ssim: NULL scratch", good, b, both, "NULL");
    b = other, b.result = nullptr, refuse ("ssim: a NULL result", good, b, both, "NULL");
    b = other, b.result = (SchroHipSsimResult *) ((char *) other.result + 4), refuse ("ssim: a misaligned result", good, b, both,
        "8-byte aligned");
    b = other, b.b_width = 40, refuse ("ssim: b narrower than a", good, b, both, "b is 40x8");
    b = other, b.scratch_bytes -= 1, refuse ("ssim: short scratch", good, b, both, "bytes of scratch");
    b = other, b.map = (double *) ((char *) other.map + 4), refuse ("ssim: a misaligned map", good, b, both, "map is not 8-byte aligned");
    b = other, b.map_stride = 8 * 47, refuse ("ssim: a short map stride", good, b, both, "map shorter than a row");
    b = other, b.scratch = good.scratch, refuse ("ssim: shared scratch", good, b, both, "share scratch");
    b = other, b.result = good.result, refuse ("ssim: a shared result", good, b, both, "share a result");
    EXPECT (schro_hip_ssim_check (nullptr, 1) == SCHRO_HIP_EINVAL && schro_hip_ssim_check (&good, 0) == SCHRO_HIP_EINVAL,
        "ssim: an empty call passes");
    EXPECT (schro_hip_ssim_batch (nullptr, &good, 1) == SCHRO_HIP_EINVAL, "ssim: no context passes");
    EXPECT (schro_hip_ssim_scratch_bytes (0, 8) == 0 && schro_hip_ssim_scratch_bytes (48, 1 << 15) == 0, "scratch for no picture");
  }

  // ---- each batch call small, larger, small, on two queues -------------------------------------------------------------
  for (int queue = 0; queue < 2; queue++) {
    EXPECT (schro_hip_context_select_queue (ctx, queue) == 0, "select queue %d", queue);
    const int sizes[3][2] = { { 3, 2 }, { 1920, 1080 }, { 65, 67 } };
    for (int s = 0; s < 3; s++) {
      const int w = sizes[s][0], h = sizes[s][1];
      size_t off = 0;
      std::vector < SchroHipSumsJob > jobs;
      for (int k = 0; k < (s == 1 ? 12 : 3); k++)
        jobs.push_back (sums_job (off, k % 2 ? w : w / 2 + 1, k % 3 ? h : h / 2 + 1, k % 4 == 3 ? 2 : 1, k % 4 < 2));
      EXPECT (schro_hip_plane_sums_batch (ctx, jobs.data (), (int) jobs.size ()) == 0, "sums of %d x %d", w, h);
      off = 0;
      std::vector < SchroHipLowpass2Plane > planes;
      for (int k = 0; k < (s == 1 ? 8 : 2); k++)
        planes.push_back (lowpass_plane (off, k % 2 ? w : w / 2 + 1, h, 1 + k % 2, sigmas[k % 6], sigmas[(k + 2) % 6]));
      EXPECT (schro_hip_lowpass2_batch (ctx, planes.data (), (int) planes.size ()) == 0, "low-pass of %d x %d", w, h);
      off = 0;
      std::vector < SchroHipSsimPicture > pics;
      for (int k = 0; k < (s == 1 ? 3 : 1); k++)
        pics.push_back (ssim_picture (off, k ? w / 2 + 1 : w, h, k != 1));
      EXPECT (schro_hip_ssim_batch (ctx, pics.data (), (int) pics.size ()) == 0, "ssim of %d x %d", w, h);
      calls += 3;
    }
  }
  {
    // the most entries a call takes, and one more
    size_t off = 0;
    std::vector < SchroHipSumsJob > jobs;
    for (int k = 0; k < 257; k++)
      jobs.push_back (sums_job (off, 5, 3, 1 + k % 2, false));
    EXPECT (schro_hip_plane_sums_batch (ctx, jobs.data (), 256) == 0, "256 sums jobs are refused");
    EXPECT (schro_hip_plane_sums_batch (ctx, jobs.data (), 257) == SCHRO_HIP_EINVAL, "257 sums jobs pass");
    off = 0;
    std::vector < SchroHipSsimPicture > pics;
    for (int k = 0; k < 65; k++)
      pics.push_back (ssim_picture (off, 9, 4, k % 2));
    EXPECT (schro_hip_ssim_batch (ctx, pics.data (), 64) == 0, "64 ssim pictures are refused");
    EXPECT (schro_hip_ssim_batch (ctx, pics.data (), 65) == SCHRO_HIP_EINVAL, "65 ssim pictures pass");
    calls += 2;
  }
  EXPECT (schro_hip_context_select_queue (ctx, 0) == 0, "select queue 0");

  // ---- the frame layer: 4:2:0 and 4:4:4, u8 and s16, small, larger, small ----------------------------------------------
  {
    const int formats[3] = { 0x03, 0x00, 0x07 };        // u8 4:2:0, u8 4:4:4, s16 4:2:0
    const int sizes[3][2] = { { 16, 8 }, { 1280, 720 }, { 33, 17 } };
    for (int s = 0; s < 3; s++)
      for (int f = 0; f < 3; f++) {
        SchroHipFrame *a = schro_hip_frame_new_and_alloc (ctx, formats[f], sizes[s][0], sizes[s][1], 0);
        SchroHipFrame *b = schro_hip_frame_new_and_alloc (ctx, formats[f], sizes[s][0], sizes[s][1], 0);
        EXPECT (a && b, "frames of %d x %d", sizes[s][0], sizes[s][1]);
        if (!a || !b)
          continue;
        for (int k = 0; k < 3; k++) {
          memset (a->components[k].data, 0x40, (size_t) a->components[k].stride * a->components[k].height);
          memset (b->components[k].data, 0x42, (size_t) b->components[k].stride * b->components[k].height);
        }
        double v = -1, mse[3] = { -1, -1, -1 };
        EXPECT (schro_hipframe_calculate_average_luma (a, &v) == 0, "average_luma");
        EXPECT (schro_hipframe_filter_lowpass2 (a, 0.75) == 0, "filter_lowpass2");
        if (f < 2) {
          EXPECT (schro_hipframe_mean_squared_error (a, b, mse) == 0, "mean_squared_error");
          EXPECT (schro_hipframe_ssim (a, b, &v) == 0, "ssim");
          EXPECT (schro_engine_get_scene_change_score_hip (a, b, 120.0, &v) == 0, "scene change score");
          EXPECT (schro_engine_get_scene_change_score_hip (a, b, 16.0, &v) == 0 && v == 1.0, "the score of a dark picture is %g", v);
        } else {
          EXPECT (schro_hipframe_mean_squared_error (a, b, mse) == SCHRO_HIP_EINVAL, "the squared error of s16 frames passes");
          EXPECT (schro_hipframe_ssim (a, b, &v) == SCHRO_HIP_EINVAL, "ssim of s16 frames passes");
        }
        schro_hip_frame_unref (a);
        schro_hip_frame_unref (b);
        calls++;
      }
    double v;
    EXPECT (schro_hipframe_calculate_average_luma (nullptr, &v) == SCHRO_HIP_EINVAL, "average_luma without a frame passes");
    EXPECT (schro_hipframe_mean_squared_error (nullptr, nullptr, &v) == SCHRO_HIP_EINVAL, "mean_squared_error without frames passes");
    EXPECT (schro_hipframe_ssim (nullptr, nullptr, &v) == SCHRO_HIP_EINVAL, "ssim without frames passes");
    EXPECT (schro_hipframe_filter_lowpass2 (nullptr, 1.0) == SCHRO_HIP_EINVAL, "filter_lowpass2 without a frame passes");
    EXPECT (schro_engine_get_scene_change_score_hip (nullptr, nullptr, 100.0, &v) == SCHRO_HIP_EINVAL, "a score without frames passes");
    EXPECT (schro_engine_get_scene_change_score_hip (nullptr, nullptr, 3.0, &v) == 0 && v == 1.0, "a dark picture needs no frames");
  }

  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  schro_hip_domain_free (ctx, block);
  schro_hip_context_free (ctx);
  printf ("picture_stats_walk: %d refusals, %d calls, %s\n", refusals, calls, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
