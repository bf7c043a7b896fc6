// mode_walk.cpp -- the host code of the whole mode decision (plane_mode.cpp, and plane_split2.cpp's refusals under it)
// walked under AddressSanitizer + UndefinedBehaviorSanitizer: a plain C++ program with its own main, linked with the
// objects of the library's device-free sanitizer build (make -C schroedinger_amd/csrc dry_asan).  Launches are dropped
// there, so what runs is every refusal, the table and scratch arithmetic and the job records of the three batch calls, over
// pictures of every geometry class: three chroma formats, one and two references, separations from 4 to 32, clipped and
// padded grids, one to eight pictures per call.  Then, on a context of its own, the frame-layer runs of the motion stages
// -- sub-pel refinement, split 2, the whole mode decision, the block-matching chain, the rough chain -- in small, large,
// small order with plane-layer calls between them: every one of them sizes the queue's scratch itself, carves fields and
// outputs out of it behind the tables and copies to and from host arrays of the exact size, so a copy out of a block
// that the batch call reallocated, or past a host field, is a report here (the CPU-side twin of
// tests/test_gpu_encoder_pipeline.py::test_scratch_sequences).  tests/test_mode_host_sanitized.py builds and runs it.
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

// ---- the frame-layer runs on a fresh context: small, large, small ---------------------------------------------------------

struct HostFields {
  std::vector < void *>owned;
  void *take (size_t bytes)
  {
    void *m = calloc (bytes ? bytes : 1, 1);    // (the exact size: a copy past it is a report)
    if (!m)
      exit (2);
    owned.push_back (m);
    return m;
  }
   ~HostFields ()
  {
    for (void *m:owned)
      free (m);
  }
};

static void
plain_frame (SchroHipContext * ctx, SchroHipFrame * f, int format, int w, int h, int ext, int upsampled)
{
  memset (f, 0, sizeof (*f));
  f->refcount = 1;
  f->domain = schro_hip_context_domain (ctx);
  f->format = format, f->width = w, f->height = h, f->extension = ext, f->is_upsampled = upsampled;
}

// the picture of `pic` as the frame layer takes it: a planar u8 frame and one upsampled frame per reference (plane images)
static void
frames_of (SchroHipContext * ctx, const Geometry & g, const Picture & pic, SchroHipFrame * src, SchroHipFrame * ups)
{
  const SchroHipSplit2Picture & s = pic.p.split2;
  const int format = g.hs | (g.vs << 1);
  plain_frame (ctx, src, format, g.w, g.h, g.ext, 0);
  for (int r = 0; r < g.refs; r++)
    plain_frame (ctx, &ups[r], format, g.w, g.h, g.ext, 1);
  for (int k = 0; k < 3; k++) {
    const int w = k ? (g.w + (1 << g.hs) - 1) >> g.hs : g.w, h = k ? (g.h + (1 << g.vs) - 1) >> g.vs : g.h;
    SchroHipFrameData d;
    memset (&d, 0, sizeof (d));
    d.format = format, d.width = w, d.height = h, d.h_shift = k ? g.hs : 0, d.v_shift = k ? g.vs : 0;
    d.data = (void *) s.src[k], d.stride = s.src_stride[k], d.length = s.src_stride[k] * h;
    src->components[k] = d;
    for (int r = 0; r < g.refs; r++) {
      d.data = (void *) s.ref_up[r][k], d.stride = s.ref_up_stride[k], d.length = 0;
      ups[r].components[k] = d;
    }
  }
}

static void
frame_layer_motion (SchroHipContext * ctx, const Geometry & g, const char *what)
{
  Picture pic;
  make (ctx, g, pic);
  SchroHipFrame src, ups[2], *up_ptrs[2] = { &ups[0], &ups[1] };
  frames_of (ctx, g, pic, &src, ups);
  const SchroHipSplit2Picture & s = pic.p.split2;
  const size_t records = (size_t) s.x_num_blocks * s.y_num_blocks;
  SchroHipParams P;
  memset (&P, 0, sizeof (P));
  P.x_num_blocks = s.x_num_blocks, P.y_num_blocks = s.y_num_blocks, P.xbsep_luma = g.xb, P.ybsep_luma = g.yb;
  P.mv_precision = g.prec, P.num_refs = g.refs;
  HostFields host;
  void *fields[2] = { nullptr, nullptr };
  const void *cfields[2], *hbm[4] = { nullptr, nullptr, nullptr, nullptr };
  for (int r = 0; r < g.refs; r++) {
    fields[r] = host.take (records * 20);
    hbm[2 * r] = host.take (records * 20);
    hbm[2 * r + 1] = host.take (records * 20);
  }
  cfields[0] = fields[0], cfields[1] = fields[1];
  void *motion = host.take (records * 20), *sb = host.take (records / 16 * 16), *trials = host.take (records / 16 * 4 * sizeof (SchroHipModeTrial));
  double stats[3];
  EXPECT (schro_encoder_motion_predict_subpel_deep_hip (&src, up_ptrs, &P, 0.1, fields) == 0, "frame-layer sub-pel refinement, %s", what);
  EXPECT (schro_mode_decision_split2_hip (&src, up_ptrs, &P, 0.1, cfields, motion, sb) == 0, "frame-layer split 2, %s", what);
  EXPECT (schro_mode_decision_hip (&src, up_ptrs, &P, 0.1, cfields, hbm, motion, sb, trials, stats) == 0, "frame-layer mode decision, %s", what);
  // the plane-layer stage behind them, on the scratch they sized
  EXPECT (schro_hip_mode_decision_batch (ctx, &pic.p, 1) == 0, "stage behind the frame-layer runs, %s", what);
  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  for (void *m:pic.owned)
    schro_hip_domain_free (ctx, m);
}

// the pyramids of a w x h 4:2:0 picture and of its reference as frames with aprons, and the two chains on them
static void
frame_layer_search (SchroHipContext * ctx, int w, int h, int ext, const char *what)
{
  const int n_levels = 3;
  std::vector < void *>owned;
  std::vector < SchroHipFrame > frames (2 * (n_levels + 1));
  SchroHipFrame *fp[n_levels + 1], *rp[n_levels + 1];
  int lw = w, lh = h;
  for (int k = 0; k <= n_levels; k++) {
    for (int side = 0; side < 2; side++) {
      SchroHipFrame *f = &frames[2 * k + side];
      plain_frame (ctx, f, 3, lw, lh, ext, 0);
      for (int c = 0; c < 3; c++) {
        const int cw = c ? (lw + 1) >> 1 : lw, ch = c ? (lh + 1) >> 1 : lh, stride = cw + 2 * ext;
        void *m = schro_hip_domain_alloc (ctx, (size_t) stride * (ch + 2 * ext));
        if (!m)
          exit (2);
        owned.push_back (m);
        SchroHipFrameData & d = f->components[c];
        d.format = 3, d.width = cw, d.height = ch, d.stride = stride, d.length = stride * (ch + 2 * ext), d.h_shift = d.v_shift = c ? 1 : 0;
        d.data = (char *) m + (size_t) ext * stride + ext;
      }
      (side ? rp : fp)[k] = f;
    }
    lw = (lw + 1) / 2, lh = (lh + 1) / 2;
  }
  SchroHipParams P;
  memset (&P, 0, sizeof (P));
  P.x_num_blocks = grid (w, 8), P.y_num_blocks = grid (h, 8), P.xbsep_luma = P.ybsep_luma = 8;
  const size_t records = (size_t) P.x_num_blocks * P.y_num_blocks;
  HostFields host;
  void *fields[n_levels + 1];
  for (int k = 0; k <= n_levels; k++)
    fields[k] = host.take (records * 20);
  EXPECT (schro_hbm_scan_hip (fp, rp, &P, n_levels, 1, 1, fields) == 0, "frame-layer block matching, %s", what);
  EXPECT (schro_hbm_scan_hip (fp, rp, &P, n_levels, 0, 0, fields) == 0, "frame-layer block matching without level 0, %s", what);
  EXPECT (schro_rough_me_heirarchical_scan_hip (fp, rp, &P, n_levels, 0, fields) == 0, "frame-layer rough chain, %s", what);
  EXPECT (schro_hierarchical_bm_scan_hint_hip (fp[1], rp[1], &P, 1, 5, 0, fields[2], fields[1]) == 0, "frame-layer block matching level, %s", what);
  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  for (void *m:owned)
    schro_hip_domain_free (ctx, m);
}

static int
frame_layer_walk ()
{
  // 16 records, then 32640, then 64: the scratch allocated from empty, grown, and reused stale by a smaller picture
  static const Geometry order[] = { {100, 75, 32, 32, 0, 0, 2, 2, 32}, {3840, 2160, 16, 16, 1, 1, 2, 2, 32}, {17, 17, 4, 4, 0, 0, 1, 1, 8} };
  static const char *const names[] = { "small", "large", "small again" };
  for (int queue = 0; queue < 2; queue++) {
    SchroHipContext *ctx = schro_hip_context_new (0);
    if (!ctx)
      return 0;
    EXPECT (schro_hip_context_select_queue (ctx, queue) == 0, "select_queue");
    for (int n = 0; n < 3; n++)
      frame_layer_motion (ctx, order[n], names[n]);
    schro_hip_context_free (ctx);
    ctx = schro_hip_context_new (0);
    if (!ctx)
      return 0;
    EXPECT (schro_hip_context_select_queue (ctx, queue) == 0, "select_queue");
    frame_layer_search (ctx, 40, 30, 32, names[0]);
    frame_layer_search (ctx, 1920, 1080, 32, names[1]);
    frame_layer_search (ctx, 64, 48, 32, names[2]);
    schro_hip_context_free (ctx);
  }
  return 3;
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
  const int walked = frame_layer_walk ();
  printf ("mode_walk: frame layer small, large, small: %d pictures on each queue, %s\n", walked, failures || !walked ? "FAILED" : "ok");
  printf ("mode_walk: %zu pictures, %s\n", pictures.size (), failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
