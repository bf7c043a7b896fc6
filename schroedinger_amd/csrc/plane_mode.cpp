// plane_mode.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: schro_mode_decision entire on the
// device -- what reads the pictures (schro_hip_mode_metric_batch), the walk (schro_hip_mode_choose_batch), the whole stage
// (schro_hip_mode_decision_batch), the refusals without a context (schro_hip_mode_decision_check) and the frame layer's run
// over host fields (mode_host_run).  The kernels are mode_decision.hip and, for the split-2 table, mode_split2.hip; the
// refusals of the split-2 stage are plane_split2.cpp's.

#include "schro_hip_internal.h"

#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr size_t kSbBytes = 16;
constexpr size_t kTrialBytes = 4 * sizeof (SchroHipModeTrial);  // per superblock
constexpr size_t kEntry2Bytes = SCHRO_HIP_SPLIT2_TABLE_INTS * sizeof (int32_t);        // per block
constexpr size_t kEntryBytes = SCHRO_HIP_MODE_TABLE_INTS * sizeof (int32_t);   // per superblock

// The refusals, and the kernels' records: `out` receives one ModeJob per picture (tables NULL where `tables` is: a stage
// call takes them from the queue's scratch).
int
build_jobs (const char *who, const SchroHipModePicture * in, int n, void *const *tables, std::vector < ModeJob > &out)
{
  SCHRO_HIP_REQUIRE (in && n > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (n <= kMaxJobs, "%s: at most %d pictures per call", who, kMaxJobs);
  std::vector < MotionSpan > spans;
  out.resize (n);
  for (int c = 0; c < n; c++) {
    const SchroHipModePicture & p = in[c];
    ModeJob & mj = out[c];
    memset (&mj, 0, sizeof (mj));
    SCHRO_HIP_REQUIRE (!tables || (tables[2 * c] && tables[2 * c + 1]), "%s: picture %d: a table is a NULL pointer", who, c);
    int r = split2_collect (who, p.split2, c, !tables, tables ? tables[2 * c] : nullptr, mj.s, spans);
    if (r)
      return r;
    const SchroHipSplit2Picture & s = p.split2;
    // (rule 12: the reference asserts in schro_get_best_split0_mv on a superblock without a source block)
    SCHRO_HIP_REQUIRE ((s.x_num_blocks - 4) * s.xbsep_luma < s.width && (s.y_num_blocks - 4) * s.ybsep_luma < s.height,
        "%s: picture %d: %d x %d blocks of %d x %d put a superblock outside the %dx%d picture", who, c, s.x_num_blocks, s.y_num_blocks, s.xbsep_luma,
        s.ybsep_luma, s.width, s.height);
    const size_t records = (size_t) s.x_num_blocks * s.y_num_blocks, superblocks = records / 16;
    for (int ref = 0; ref < s.num_refs; ref++)
      for (int level = 0; level < 2; level++) {
        const void *f = p.hbm_fields[ref][level];
        SCHRO_HIP_REQUIRE (f, "%s: picture %d: the level-%d field of reference %d is a NULL pointer", who, c, level + 1, ref);
        SCHRO_HIP_REQUIRE (((uintptr_t) f & 3) == 0, "%s: picture %d: the level-%d field of reference %d is not 4-byte aligned", who, c, level + 1, ref);
        spans.push_back ({(uintptr_t) f, (uintptr_t) f + records * kMvBytes, false, c, -1, level ? "a level-2 field" : "a level-1 field"});
        mj.hbm[ref][level] = (const uint8_t *) f;
      }
    SCHRO_HIP_REQUIRE (p.trials && p.stats, "%s: picture %d: the trial table or the statistics are a NULL pointer", who, c);
    SCHRO_HIP_REQUIRE (((uintptr_t) p.trials & 7) == 0 && ((uintptr_t) p.stats & 7) == 0, "%s: picture %d: the trial table or the statistics are not 8-byte aligned",
        who, c);
    spans.push_back ({(uintptr_t) p.trials, (uintptr_t) p.trials + superblocks * kTrialBytes, true, c, -1, "the trial table"});
    spans.push_back ({(uintptr_t) p.stats, (uintptr_t) p.stats + 3 * sizeof (double), true, c, -1, "the statistics"});
    if (tables) {
      SCHRO_HIP_REQUIRE (((uintptr_t) tables[2 * c + 1] & 3) == 0, "%s: picture %d: the mode table is not 4-byte aligned", who, c);
      spans.push_back ({(uintptr_t) tables[2 * c + 1], (uintptr_t) tables[2 * c + 1] + superblocks * kEntryBytes, true, c, -1, "the mode table"});
      mj.table = (int32_t *) tables[2 * c + 1];
    }
    mj.trials = (uint8_t *) p.trials;
    mj.stats = (double *) p.stats;
  }
  return motion_check_spans (who, "picture", spans);
}

// the workgroups of the two metric launches, picture by picture; `split2` receives the split-2 stage's records
void
lay_out (std::vector < ModeJob > &jobs, std::vector < Split2Job > &split2, int *groups2, int *groups)
{
  const int per2 = split2_metric_blocks (), units = mode_metric_units (), per = mode_metric_waves ();
  *groups2 = 0, *groups = 0;
  split2.resize (jobs.size ());
  for (size_t c = 0; c < jobs.size (); c++) {
    const int blocks = jobs[c].s.nbx * jobs[c].s.nby;
    jobs[c].s.tile_base = *groups2;
    *groups2 += (blocks + per2 - 1) / per2;
    jobs[c].tile_base = *groups;
    *groups += (blocks / 16 * units + per - 1) / per;
    split2[c] = jobs[c].s;
  }
}

int
run (SchroHipContext * ctx, std::vector < ModeJob > &jobs, bool metric, bool choose)
{
  std::vector < Split2Job > split2;
  int groups2, groups;
  lay_out (jobs, split2, &groups2, &groups);
  const int n = (int) jobs.size ();
  void *dev, *dev2;
  int r = push_big_table (ctx, jobs.data (), sizeof (ModeJob) * jobs.size (), &dev);
  if (r)
    return r;
  if (metric) {
    r = push_big_table (ctx, split2.data (), sizeof (Split2Job) * split2.size (), &dev2);
    if (r)
      return r;
    r = launch_split2_metric (ctx->stream, (const Split2Job *) dev2, n, groups2);
    if (r)
      return r;
    r = launch_mode_metric (ctx->stream, (const ModeJob *) dev, n, groups);
    if (r)
      return r;
  }
  return choose ? launch_mode_choose (ctx->stream, (const ModeJob *) dev, n) : 0;
}

}                               // namespace

extern "C" {

int
schro_hip_mode_decision_check (const SchroHipModePicture * pictures, int n)
{
  std::vector < ModeJob > out;
  return build_jobs ("mode_decision_batch", pictures, n, nullptr, out);
}

int
schro_hip_mode_metric_batch (SchroHipContext * ctx, const SchroHipModePicture * pictures, int n, void *const *tables)
{
  SCHRO_HIP_REQUIRE (ctx && tables, "mode_metric_batch: bad arguments");
  std::vector < ModeJob > out;
  int r = build_jobs ("mode_metric_batch", pictures, n, tables, out);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);
  return run (ctx, out, true, false);
}

int
schro_hip_mode_choose_batch (SchroHipContext * ctx, const SchroHipModePicture * pictures, int n, void *const *tables)
{
  SCHRO_HIP_REQUIRE (ctx && tables, "mode_choose_batch: bad arguments");
  std::vector < ModeJob > out;
  int r = build_jobs ("mode_choose_batch", pictures, n, tables, out);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);
  return run (ctx, out, false, true);
}

int
schro_hip_mode_decision_batch (SchroHipContext * ctx, const SchroHipModePicture * pictures, int n)
{
  const char *who = "mode_decision_batch";
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  std::vector < ModeJob > out;
  int r = build_jobs (who, pictures, n, nullptr, out);
  if (r)
    return r;
  // the tables: two slots of the queue's scratch per picture
  size_t need = 0;
  std::vector < size_t > slot (2 * n, 0);
  for (int c = 0; c < n; c++) {
    const size_t records = (size_t) out[c].s.nbx * out[c].s.nby;
    slot[2 * c] = need;
    need += round_up (records * kEntry2Bytes, 256);
    slot[2 * c + 1] = need;
    need += round_up (records / 16 * kEntryBytes, 256);
  }
  (void) hipSetDevice (ctx->device);
  r = ensure_scratch (ctx, need);
  if (r)
    return r;
  for (int c = 0; c < n; c++) {
    out[c].s.table = (int32_t *) ((uint8_t *) ctx->scratch_ref () + slot[2 * c]);
    out[c].table = (int32_t *) ((uint8_t *) ctx->scratch_ref () + slot[2 * c + 1]);
  }
  return run (ctx, out, true, true);
}

}                               // extern "C"

namespace schro {

int
mode_host_run (SchroHipContext * ctx, SchroHipModePicture * pic, void *motion, void *superblocks, void *trials, double *stats)
{
  // the fields and the outputs: slots of the queue's scratch BEHIND the tables schro_hip_mode_decision_batch takes from its
  // start -- so the scratch is sized here for all of them and the batch finds it large enough
  SchroHipSplit2Picture & s = pic->split2;
  const size_t records = (size_t) std::max (s.x_num_blocks, 0) * std::max (s.y_num_blocks, 0), superblocks_n = records / 16;
  const size_t tables = round_up (records * kEntry2Bytes, 256) + round_up (superblocks_n * kEntryBytes, 256);
  const size_t field = round_up (records * kMvBytes, 256), sb = round_up (superblocks_n * kSbBytes + 8, 256);
  const size_t tr = round_up (superblocks_n * kTrialBytes + 8, 256);
  (void) hipSetDevice (ctx->device);
  int r = ensure_scratch (ctx, tables + 7 * field + sb + tr + 512);
  if (r)
    return r;
  uint8_t *base = (uint8_t *) ctx->scratch_ref () + tables;
  const void *host[2] = { s.fields[0], s.fields[1] };
  const void *host_hbm[2][2] = { {pic->hbm_fields[0][0], pic->hbm_fields[0][1]}, {pic->hbm_fields[1][0], pic->hbm_fields[1][1]} };
  const int nrefs = std::min (std::max (s.num_refs, 0), 2);
  for (int k = 0; k < nrefs; k++) {
    s.fields[k] = base + k * field;
    for (int level = 0; level < 2; level++)
      pic->hbm_fields[k][level] = host_hbm[k][level] ? base + (2 + 2 * k + level) * field : nullptr;
  }
  s.motion = base + 6 * field;
  s.superblocks = base + 7 * field;
  pic->trials = base + 7 * field + sb;
  pic->stats = base + 7 * field + sb + tr;
  // (refused before anything is copied)
  r = schro_hip_mode_decision_check (pic, 1);
  if (r)
    return r;
  for (int k = 0; k < nrefs; k++) {
    SCHRO_HIP_CHECK (hipMemcpyAsync ((void *) s.fields[k], host[k], records * kMvBytes, hipMemcpyHostToDevice, ctx->stream));
    for (int level = 0; level < 2; level++)
      SCHRO_HIP_CHECK (hipMemcpyAsync ((void *) pic->hbm_fields[k][level], host_hbm[k][level], records * kMvBytes, hipMemcpyHostToDevice, ctx->stream));
  }
  r = schro_hip_mode_decision_batch (ctx, pic, 1);
  if (r)
    return r;
  SCHRO_HIP_CHECK (hipMemcpyAsync (motion, s.motion, records * kMvBytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipMemcpyAsync (superblocks, s.superblocks, superblocks_n * kSbBytes, hipMemcpyDeviceToHost, ctx->stream));
  if (trials)
    SCHRO_HIP_CHECK (hipMemcpyAsync (trials, pic->trials, superblocks_n * kTrialBytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipMemcpyAsync (stats, pic->stats, 3 * sizeof (double), hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

}                               // namespace schro
