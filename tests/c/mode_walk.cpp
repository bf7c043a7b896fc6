// mode_walk.cpp -- the host code of the whole mode decision (plane_mode.cpp, and plane_split2.cpp's refusals under it)
// walked under AddressSanitizer + UndefinedBehaviorSanitizer: a plain C++ program with its own main, linked with the
// objects of the library's device-free sanitizer build (make -C schroedinger_amd/csrc dry_asan).  Launches are dropped
// there, so what runs is every refusal, the table and scratch arithmetic and the job records of the three batch calls, over
// pictures of every geometry class: three chroma formats, one and two references, separations from 4 to 32, clipped and
// padded grids, one to eight pictures per call.  tests/test_mode_host_sanitized.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "mode_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

struct Geometry {
  int w, h, xb, yb, hs, vs, prec, refs, ext;
};

struct Picture {
  SchroHipModePicture p;
  std::vector < void *>owned;
  void *tables[2];
};

static int
grid (int size, int b)
{
  return ((size + b - 1) / b + 3) / 4 * 4;
}

static void *
take (SchroHipContext * ctx, Picture & pic, size_t bytes)
{
  void *m = schro_hip_domain_alloc (ctx, bytes + 256);
  if (!m) {
    fprintf (stderr, "mode_walk: no memory: %s\n", schro_hip_last_error ());
    exit (2);
  }
  pic.owned.push_back (m);
  return m;
}

static void
make (SchroHipContext * ctx, const Geometry & g, Picture & pic)
{
  memset (&pic.p, 0, sizeof (pic.p));
  SchroHipSplit2Picture & s = pic.p.split2;
  s.width = g.w, s.height = g.h, s.h_shift = g.hs, s.v_shift = g.vs, s.extension = g.ext;
  s.xbsep_luma = g.xb, s.ybsep_luma = g.yb, s.mv_precision = g.prec, s.num_refs = g.refs, s.lambda = 0.1;
  s.x_num_blocks = grid (g.w, g.xb), s.y_num_blocks = grid (g.h, g.yb);
  const size_t records = (size_t) s.x_num_blocks * s.y_num_blocks;
  for (int k = 0; k < 3; k++) {
    const int w = k ? (g.w + (1 << g.hs) - 1) >> g.hs : g.w, h = k ? (g.h + (1 << g.vs) - 1) >> g.vs : g.h;
    s.src_stride[k] = w + 5;
    s.src[k] = (const uint8_t *) take (ctx, pic, (size_t) s.src_stride[k] * h);
    int stride = 0;
    const size_t bytes = schro_hip_upsampled_bytes (w, h, &stride);
    s.ref_up_stride[k] = stride;
    for (int r = 0; r < g.refs; r++)
      s.ref_up[r][k] = (const uint8_t *) take (ctx, pic, bytes);
  }
  for (int r = 0; r < g.refs; r++) {
    s.fields[r] = take (ctx, pic, records * 20);
    pic.p.hbm_fields[r][0] = take (ctx, pic, records * 20);
    pic.p.hbm_fields[r][1] = take (ctx, pic, records * 20);
  }
  s.motion = take (ctx, pic, records * 20);
  s.superblocks = take (ctx, pic, records);
  pic.p.trials = take (ctx, pic, records / 16 * 4 * sizeof (SchroHipModeTrial));
  pic.p.stats = take (ctx, pic, 24);
  pic.tables[0] = take (ctx, pic, records * SCHRO_HIP_SPLIT2_TABLE_INTS * 4);
  pic.tables[1] = take (ctx, pic, records / 16 * SCHRO_HIP_MODE_TABLE_INTS * 4);
}

static void
refusals (const SchroHipModePicture & good)
{
  SchroHipModePicture two[2] = { good, good };
  // (two copies of one picture overlap in their outputs: that alone is the first refusal)
  EXPECT (schro_hip_mode_decision_check (two, 2) == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), "overlaps"), "two pictures with one motion field pass");
  struct {
    const char *word;
    void (*spoil) (SchroHipModePicture &);
  } const rows[] = {
    {"level-1 field",[](SchroHipModePicture & p) { p.hbm_fields[0][0] = nullptr; }},
    {"level-2 field",[](SchroHipModePicture & p) { p.hbm_fields[0][1] = nullptr; }},
    {"not 4-byte aligned",[](SchroHipModePicture & p) { p.hbm_fields[0][1] = (const char *) p.hbm_fields[0][1] + 2; }},
    {"trial table",[](SchroHipModePicture & p) { p.trials = nullptr; }},
    {"statistics",[](SchroHipModePicture & p) { p.stats = nullptr; }},
    {"8-byte aligned",[](SchroHipModePicture & p) { p.stats = (char *) p.stats + 4; }},
    {"superblock outside",[](SchroHipModePicture & p) { p.split2.x_num_blocks += 4; }},
    {"superblock outside",[](SchroHipModePicture & p) { p.split2.y_num_blocks += 4; }},
    {"whole superblocks",[](SchroHipModePicture & p) { p.split2.x_num_blocks += 2; }},
    {"blocks",[](SchroHipModePicture & p) { p.split2.y_num_blocks = 0x7ffffffc; }},
    {"mv_precision",[](SchroHipModePicture & p) { p.split2.mv_precision = 4; }},
    {"extension",[](SchroHipModePicture & p) { p.split2.extension = 33; }},
    {"lambda",[](SchroHipModePicture & p) { p.split2.lambda = -1; }},
    {"references",[](SchroHipModePicture & p) { p.split2.num_refs = 3; }},
    {"picture size",[](SchroHipModePicture & p) { p.split2.width = 0x7fffffff; }},
    {"overlaps",[](SchroHipModePicture & p) { p.trials = p.split2.motion; }},
    {"overlaps",[](SchroHipModePicture & p) { p.stats = (void *) p.hbm_fields[0][0]; }},
    {"overlaps",[](SchroHipModePicture & p) { p.split2.superblocks = (char *) p.trials + 8; }},
    {"NULL",[](SchroHipModePicture & p) { p.split2.motion = nullptr; }},
  };
  for (const auto & row:rows) {
    SchroHipModePicture bad = good;
    row.spoil (bad);
    const int r = schro_hip_mode_decision_check (&bad, 1);
    EXPECT (r == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), "picture 0") && strstr (schro_hip_last_error (), row.word), "`%s` is not refused as such", row.word);
  }
  EXPECT (schro_hip_mode_decision_check (nullptr, 1) == SCHRO_HIP_EINVAL, "no pictures pass");
  EXPECT (schro_hip_mode_decision_check (&good, 0) == SCHRO_HIP_EINVAL, "zero pictures pass");
  EXPECT (schro_hip_mode_decision_check (&good, 1 << 20) == SCHRO_HIP_EINVAL, "2^20 pictures pass");
}

int
main ()
{
  static const Geometry geometries[] = {
    {96, 96, 8, 8, 1, 1, 2, 2, 32}, {48, 48, 4, 4, 1, 1, 3, 2, 4}, {100, 75, 32, 32, 0, 0, 2, 2, 32}, {160, 96, 16, 8, 1, 0, 2, 2, 16},
    {104, 88, 8, 8, 1, 1, 1, 1, 32}, {101, 75, 8, 8, 1, 1, 0, 2, 32}, {17, 17, 4, 4, 0, 0, 0, 1, 8}, {3840, 2160, 16, 16, 1, 1, 2, 2, 32},
  };
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "mode_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
    return 2;
  }
  std::vector < Picture > pictures (sizeof (geometries) / sizeof (geometries[0]));
  for (size_t n = 0; n < pictures.size (); n++)
    make (ctx, geometries[n], pictures[n]);
  for (size_t n = 0; n < pictures.size (); n++) {
    EXPECT (schro_hip_mode_decision_check (&pictures[n].p, 1) == 0, "picture %zu is refused", n);
    refusals (pictures[n].p);
  }
  // batches of 1 .. all pictures through the three calls (the launches themselves are dropped in this build)
  for (size_t count = 1; count <= pictures.size (); count++) {
    std::vector < SchroHipModePicture > batch;
    std::vector < void *>tables;
    for (size_t n = 0; n < count; n++) {
      batch.push_back (pictures[n].p);
      tables.push_back (pictures[n].tables[0]);
      tables.push_back (pictures[n].tables[1]);
    }
    EXPECT (schro_hip_mode_metric_batch (ctx, batch.data (), (int) count, tables.data ()) == 0, "metric batch of %zu", count);
    EXPECT (schro_hip_mode_choose_batch (ctx, batch.data (), (int) count, tables.data ()) == 0, "choice batch of %zu", count);
    EXPECT (schro_hip_mode_decision_batch (ctx, batch.data (), (int) count) == 0, "stage of %zu", count);
    // a table that is another picture's, a missing one
    if (count > 1) {
      std::vector < void *>spoilt = tables;
      spoilt[3] = spoilt[1];
      EXPECT (schro_hip_mode_metric_batch (ctx, batch.data (), (int) count, spoilt.data ()) == SCHRO_HIP_EINVAL, "one mode table for two pictures passes");
      spoilt[3] = nullptr;
      EXPECT (schro_hip_mode_choose_batch (ctx, batch.data (), (int) count, spoilt.data ()) == SCHRO_HIP_EINVAL, "a missing table passes");
    }
  }
  EXPECT (schro_hip_mode_metric_batch (nullptr, &pictures[0].p, 1, pictures[0].tables) == SCHRO_HIP_EINVAL, "no context passes");
  EXPECT (schro_hip_mode_decision_batch (nullptr, &pictures[0].p, 1) == SCHRO_HIP_EINVAL, "no context passes");
  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  for (Picture & pic:pictures)
    for (void *m:pic.owned)
      schro_hip_domain_free (ctx, m);
  schro_hip_context_free (ctx);
  printf ("mode_walk: %zu pictures, %s\n", pictures.size (), failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
