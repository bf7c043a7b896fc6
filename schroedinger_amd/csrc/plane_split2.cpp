// plane_split2.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: the split-2 level of the mode
// decision on the device, schro_do_split2 -- what reads the pictures (schro_hip_split2_metric_batch), the choice
// (schro_hip_split2_choose_batch), the whole stage (schro_hip_split2_batch), the refusals without a context
// (schro_hip_split2_check) and the frame layer's run over host fields (split2_host_run).  The kernels are mode_split2.hip.

#include "schro_hip_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr size_t kSbBytes = 16; // int32 error, int32 entropy, double score
constexpr size_t kEntryBytes = SCHRO_HIP_SPLIT2_TABLE_INTS * sizeof (int32_t);

enum Call { kMetric, kChoose, kStage };

}                               // namespace

namespace schro {

// The refusals of one picture but for the overlaps, its kernel record and its spans (the table's too where `table` is
// given).
int
split2_collect (const char *who, const SchroHipSplit2Picture & s, int c, bool stage, void *table, Split2Job & jb, std::vector < MotionSpan > &spans)
{
  static const char *const comp[3] = { "Y", "U", "V" };
  const char *what = "picture";
  const Call call = stage ? kStage : kMetric;
  {
    SCHRO_HIP_REQUIRE (s.num_refs == 1 || s.num_refs == 2, "%s: picture %d: %d references, neither 1 nor 2", who, c, s.num_refs);
    SCHRO_HIP_REQUIRE ((s.h_shift == 0 || s.h_shift == 1) && (s.v_shift == 0 || s.v_shift == 1) && s.v_shift <= s.h_shift,
        "%s: picture %d: chroma shifts %d,%d are none of 0,0 / 1,0 / 1,1", who, c, s.h_shift, s.v_shift);
    int r = motion_check_blocks (who, what, c, s.x_num_blocks, s.y_num_blocks);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (s.x_num_blocks % 4 == 0 && s.y_num_blocks % 4 == 0, "%s: picture %d: %d x %d blocks are not whole superblocks", who, c,
        s.x_num_blocks, s.y_num_blocks);
    r = motion_check_block_size (who, what, c, s.xbsep_luma, s.ybsep_luma, kMaxTiledBlock);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (s.xbsep_luma % (1 << s.h_shift) == 0 && s.ybsep_luma % (1 << s.v_shift) == 0,
        "%s: picture %d: a block of %d x %d is no multiple of the chroma subsampling", who, c, s.xbsep_luma, s.ybsep_luma);
    r = motion_check_precision (who, what, c, s.mv_precision);
    if (!r)
      r = motion_check_picture (who, what, c, s.width, s.height, s.xbsep_luma, s.ybsep_luma, s.extension, s.mv_precision, s.lambda);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (s.motion && s.superblocks, "%s: picture %d: the motion field or the superblock table is a NULL pointer", who, c);
    SCHRO_HIP_REQUIRE (call == kStage || table, "%s: picture %d: the table is a NULL pointer", who, c);
    SCHRO_HIP_REQUIRE (((uintptr_t) s.motion & 3) == 0 && ((uintptr_t) s.superblocks & 7) == 0 && (call == kStage || ((uintptr_t) table & 3) == 0),
        "%s: picture %d: the motion field or the table is not 4-byte aligned, or the superblock table not 8-byte aligned", who, c);
    const size_t records = (size_t) s.x_num_blocks * s.y_num_blocks;
    const int cw = (s.width + (1 << s.h_shift) - 1) >> s.h_shift, ch = (s.height + (1 << s.v_shift) - 1) >> s.v_shift;
    const bool pair = s.chroma_pairs != 0;
    SCHRO_HIP_REQUIRE (!pair || s.h_shift == 1, "%s: picture %d: only a horizontally subsampled picture has pair images", who, c);
    memset (&jb, 0, sizeof (jb));
    for (int k = 0; k < 3; k++) {
      const int w = k ? cw : s.width, h = k ? ch : s.height;
      SCHRO_HIP_REQUIRE (s.src[k], "%s: picture %d: component %s of the picture is a NULL pointer", who, c, comp[k]);
      SCHRO_HIP_REQUIRE (s.src_stride[k] >= w, "%s: picture %d: component %s: stride %d is shorter than a row of %d", who, c, comp[k],
          s.src_stride[k], w);
      spans.push_back ({(uintptr_t) s.src[k], (uintptr_t) s.src[k] + (size_t) s.src_stride[k] * (h - 1) + w, false, c, -1, "the picture"});
      jb.src[k] = s.src[k];
      jb.src_stride[k] = s.src_stride[k];
      if (pair && k == 2)
        continue;
      int up_stride = 0;
      const size_t up_bytes = pair && k ? schro_hip_upsampled_pair_bytes (w, h, &up_stride) : schro_hip_upsampled_bytes (w, h, &up_stride);
      SCHRO_HIP_REQUIRE (s.ref_up_stride[k] == up_stride, "%s: picture %d: the upsampled %s image has a stride of %d, a %dx%d component has %d", who,
          c, comp[k], s.ref_up_stride[k], w, h, up_stride);
      for (int r = 0; r < s.num_refs; r++) {
        SCHRO_HIP_REQUIRE (s.ref_up[r][k], "%s: picture %d: the upsampled %s image of reference %d is a NULL pointer", who, c, comp[k], r);
        SCHRO_HIP_REQUIRE (((uintptr_t) s.ref_up[r][k] & 127) == 0, "%s: picture %d: the upsampled %s image of reference %d is not 128-byte aligned",
            who, c, comp[k], r);
        spans.push_back ({(uintptr_t) s.ref_up[r][k], (uintptr_t) s.ref_up[r][k] + up_bytes, false, c, -1, "an upsampled image"});
        jb.up[r][k] = s.ref_up[r][k];
      }
      if (k < 2)
        jb.up_stride[k] = s.ref_up_stride[k];
    }
    for (int r = 0; r < s.num_refs; r++) {
      SCHRO_HIP_REQUIRE (s.fields[r], "%s: picture %d: the field of reference %d is a NULL pointer", who, c, r);
      SCHRO_HIP_REQUIRE (((uintptr_t) s.fields[r] & 3) == 0, "%s: picture %d: the field of reference %d is not 4-byte aligned", who, c, r);
      spans.push_back ({(uintptr_t) s.fields[r], (uintptr_t) s.fields[r] + records * kMvBytes, false, c, -1, "a sub-pel field"});
      jb.field[r] = (const uint8_t *) s.fields[r];
    }
    spans.push_back ({(uintptr_t) s.motion, (uintptr_t) s.motion + records * kMvBytes, true, c, -1, "the motion field"});
    spans.push_back ({(uintptr_t) s.superblocks, (uintptr_t) s.superblocks + records / 16 * kSbBytes, true, c, -1, "the superblock table"});
    if (call != kStage)
      spans.push_back ({(uintptr_t) table, (uintptr_t) table + records * kEntryBytes, true, c, -1, "the table"});
    jb.motion = (uint8_t *) s.motion;
    jb.sb = (uint8_t *) s.superblocks;
    jb.table = call == kStage ? nullptr : (int32_t *) table;
    jb.lambda = s.lambda;
    jb.w = s.width, jb.h = s.height, jb.cw = cw, jb.ch = ch, jb.ext = s.extension;
    jb.nbx = s.x_num_blocks, jb.nby = s.y_num_blocks, jb.xb = s.xbsep_luma, jb.yb = s.ybsep_luma;
    jb.hs = s.h_shift, jb.vs = s.v_shift, jb.prec = s.mv_precision, jb.num_refs = s.num_refs;
    jb.pair = pair;
  }
  return 0;
}

}                               // namespace schro

namespace {

// The refusals, and the kernels' records: `out` receives one Split2Job per picture (table NULL where `tables` is).
int
build_jobs (const char *who, Call call, const SchroHipSplit2Picture * in, int n, void *const *tables, std::vector < Split2Job > &out)
{
  SCHRO_HIP_REQUIRE (in && n > 0 && (call == kStage || tables), "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (n <= kMaxJobs, "%s: at most %d pictures per call", who, kMaxJobs);
  std::vector < MotionSpan > spans;
  out.resize (n);
  for (int c = 0; c < n; c++) {
    const int r = split2_collect (who, in[c], c, call == kStage, call == kStage ? nullptr : tables[c], out[c], spans);
    if (r)
      return r;
  }
  return motion_check_spans (who, "picture", spans);
}

// the workgroups of the metric launch, picture by picture; returns their number
int
lay_out (Split2Job * jobs, int n)
{
  const int per = split2_metric_blocks ();
  int total = 0;
  for (int c = 0; c < n; c++) {
    jobs[c].tile_base = total;
    total += (jobs[c].nbx * jobs[c].nby + per - 1) / per;
  }
  return total;
}

}                               // namespace

extern "C" {

int
schro_hip_split2_check (const SchroHipSplit2Picture * pictures, int n)
{
  std::vector < Split2Job > out;
  return build_jobs ("split2_batch", kStage, pictures, n, nullptr, out);
}

int
schro_hip_split2_metric_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n, void *const *tables)
{
  SCHRO_HIP_REQUIRE (ctx, "split2_metric_batch: bad arguments");
  std::vector < Split2Job > out;
  int r = build_jobs ("split2_metric_batch", kMetric, pictures, n, tables, out);
  if (r)
    return r;
  const int total = lay_out (out.data (), n);
  (void) hipSetDevice (ctx->device);
  void *dev;
  r = push_big_table (ctx, out.data (), sizeof (Split2Job) * out.size (), &dev);
  return r ? r : launch_split2_metric (ctx->stream, (const Split2Job *) dev, n, total);
}

int
schro_hip_split2_choose_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n, void *const *tables)
{
  SCHRO_HIP_REQUIRE (ctx, "split2_choose_batch: bad arguments");
  std::vector < Split2Job > out;
  int r = build_jobs ("split2_choose_batch", kChoose, pictures, n, tables, out);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);
  void *dev;
  r = push_big_table (ctx, out.data (), sizeof (Split2Job) * out.size (), &dev);
  return r ? r : launch_split2_choose (ctx->stream, (const Split2Job *) dev, n);
}

int
schro_hip_split2_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n)
{
  const char *who = "split2_batch";
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  std::vector < Split2Job > out;
  int r = build_jobs (who, kStage, pictures, n, nullptr, out);
  if (r)
    return r;
  // the tables: a slot of the queue's scratch per picture
  size_t need = 0;
  std::vector < size_t > slot (n, 0);
  for (int c = 0; c < n; c++) {
    slot[c] = need;
    need += round_up ((size_t) out[c].nbx * out[c].nby * kEntryBytes, 256);
  }
  (void) hipSetDevice (ctx->device);
  r = ensure_scratch (ctx, need);
  if (r)
    return r;
  for (int c = 0; c < n; c++)
    out[c].table = (int32_t *) ((uint8_t *) ctx->scratch_ref () + slot[c]);
  const int total = lay_out (out.data (), n);
  void *dev;
  r = push_big_table (ctx, out.data (), sizeof (Split2Job) * out.size (), &dev);
  if (r)
    return r;
  r = launch_split2_metric (ctx->stream, (const Split2Job *) dev, n, total);
  return r ? r : launch_split2_choose (ctx->stream, (const Split2Job *) dev, n);
}

}                               // extern "C"

namespace schro {

int
split2_host_run (SchroHipContext * ctx, SchroHipSplit2Picture * pic, void *motion, void *superblocks)
{
  // the fields and the outputs: slots of the queue's scratch BEHIND the table schro_hip_split2_batch takes from its start
  // -- so the scratch is sized here for all of them and the batch finds it large enough
  const size_t records = (size_t) std::max (pic->x_num_blocks, 0) * std::max (pic->y_num_blocks, 0);
  const size_t table = round_up (records * kEntryBytes, 256), field = round_up (records * kMvBytes, 256), sb = round_up (records / 16 * kSbBytes + 8, 256);
  (void) hipSetDevice (ctx->device);
  int r = ensure_scratch (ctx, table + 3 * field + sb + 256);
  if (r)
    return r;
  uint8_t *base = (uint8_t *) ctx->scratch_ref () + table;
  const void *host[2] = { pic->fields[0], pic->fields[1] };
  const int nrefs = std::min (std::max (pic->num_refs, 0), 2);
  for (int k = 0; k < nrefs; k++)
    pic->fields[k] = base + k * field;
  pic->motion = base + 2 * field;
  pic->superblocks = base + 3 * field;
  // (refused before anything is copied)
  r = schro_hip_split2_check (pic, 1);
  if (r)
    return r;
  for (int k = 0; k < nrefs; k++)
    SCHRO_HIP_CHECK (hipMemcpyAsync ((void *) pic->fields[k], host[k], records * kMvBytes, hipMemcpyHostToDevice, ctx->stream));
  r = schro_hip_split2_batch (ctx, pic, 1);
  if (r)
    return r;
  SCHRO_HIP_CHECK (hipMemcpyAsync (motion, pic->motion, records * kMvBytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipMemcpyAsync (superblocks, pic->superblocks, records / 16 * kSbBytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

}                               // namespace schro
