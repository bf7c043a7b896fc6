// plane_subpel.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: sub-pel motion refinement on the
// device, schro_encoder_motion_predict_subpel_deep -- one pass's errors (schro_hip_subpel_error_batch), one pass's choice
// (schro_hip_subpel_choose_batch), the whole stage (schro_hip_subpel_batch), the refusals without a context
// (schro_hip_subpel_check) and the frame layer's run over host fields (subpel_host_run).  The kernels are subpel.hip.

#include "schro_hip_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

enum Call { kError, kChoose, kStage };

// The refusals, and the kernels' records: `out` receives one SubpelChain per chain (table NULL where `tables` is).
// mvprec: the pass of the error and choice calls (checked against the chain's precision); 0 for the whole stage.
int
build_chains (const char *who, Call call, const SchroHipSubpelChain * in, int nchains, int mvprec, void *const *tables,
    std::vector < SubpelChain > &out)
{
  const char *what = "chain";
  SCHRO_HIP_REQUIRE (in && nchains > 0 && (call == kStage || tables), "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (nchains <= kMaxJobs, "%s: at most %d chains per call", who, kMaxJobs);
  std::vector < MotionSpan > spans;
  out.resize (nchains);
  for (int c = 0; c < nchains; c++) {
    const SchroHipSubpelChain & s = in[c];
    const MotionGeometry g = { s.x_num_blocks, s.y_num_blocks, s.xbsep_luma, s.ybsep_luma, s.ref_index };
    int r = motion_check_geometry (who, what, c, g, kMaxTiledBlock);
    if (!r)
      r = motion_check_precision (who, what, c, s.mv_precision);
    if (r)
      return r;
    if (call != kStage)
      SCHRO_HIP_REQUIRE (mvprec >= 1 && mvprec <= s.mv_precision, "%s: chain %d: pass %d is outside 1 .. mv_precision %d", who, c, mvprec,
          s.mv_precision);
    r = motion_check_picture (who, what, c, s.width, s.height, s.xbsep_luma, s.ybsep_luma, s.extension, s.mv_precision, s.lambda);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (s.src && s.ref_up, "%s: chain %d: the picture or the upsampled image is a NULL pointer", who, c);
    SCHRO_HIP_REQUIRE (s.field && (call != kStage || s.src_field), "%s: chain %d: a field is a NULL pointer", who, c);
    SCHRO_HIP_REQUIRE (call == kStage || tables[c], "%s: chain %d: the table is a NULL pointer", who, c);
    SCHRO_HIP_REQUIRE (s.src_stride >= s.width, "%s: chain %d: stride %d is shorter than a row of %d", who, c, s.src_stride, s.width);
    int up_stride = 0;
    const size_t up_bytes = schro_hip_upsampled_bytes (s.width, s.height, &up_stride);
    SCHRO_HIP_REQUIRE (((uintptr_t) s.ref_up & 127) == 0, "%s: chain %d: the upsampled image is not 128-byte aligned", who, c);
    SCHRO_HIP_REQUIRE (s.ref_up_stride == up_stride, "%s: chain %d: the upsampled image has a stride of %d, a %dx%d component has %d", who, c,
        s.ref_up_stride, s.width, s.height, up_stride);
    SCHRO_HIP_REQUIRE (((uintptr_t) s.field & 3) == 0 && (call != kStage || ((uintptr_t) s.src_field & 3) == 0)
        && (call == kStage || ((uintptr_t) tables[c] & 3) == 0), "%s: chain %d: a field or table is not 4-byte aligned", who, c);
    const size_t records = (size_t) s.x_num_blocks * s.y_num_blocks, bytes = records * kMvBytes;
    spans.push_back ({(uintptr_t) s.src, (uintptr_t) s.src + (size_t) s.src_stride * (s.height - 1) + s.width, false, c, -1, "the picture"});
    spans.push_back ({(uintptr_t) s.ref_up, (uintptr_t) s.ref_up + up_bytes, false, c, -1, "the upsampled image"});
    spans.push_back ({(uintptr_t) s.field, (uintptr_t) s.field + bytes, true, c, -1, "the field"});
    if (call == kStage && s.src_field != s.field)
      spans.push_back ({(uintptr_t) s.src_field, (uintptr_t) s.src_field + bytes, false, c, -1, "the source field"});
    if (call != kStage)
      spans.push_back ({(uintptr_t) tables[c], (uintptr_t) tables[c] + records * 8 * sizeof (int32_t), true, c, -1, "the table"});
    SubpelChain & ch = out[c];
    memset (&ch, 0, sizeof (ch));
    ch.src = s.src;
    ch.up = s.ref_up;
    ch.field = (uint8_t *) s.field;
    ch.table = call == kStage ? nullptr : (int32_t *) tables[c];
    ch.lambda = s.lambda;
    ch.src_stride = s.src_stride;
    ch.up_stride = s.ref_up_stride;
    ch.w = s.width, ch.h = s.height, ch.ext = s.extension;
    ch.nbx = s.x_num_blocks, ch.nby = s.y_num_blocks, ch.xb = s.xbsep_luma, ch.yb = s.ybsep_luma;
    ch.ref = s.ref_index;
  }
  return motion_check_spans (who, what, spans);
}

// the workgroups of the error launch, chain by chain; returns their number
int
lay_out (SubpelChain * chains, int n)
{
  const int per = subpel_error_blocks ();
  int total = 0;
  for (int c = 0; c < n; c++) {
    chains[c].tile_base = total;
    total += (chains[c].nbx * chains[c].nby + per - 1) / per;
  }
  return total;
}

}                               // namespace

extern "C" {

int
schro_hip_subpel_check (const SchroHipSubpelChain * chains, int nchains)
{
  std::vector < SubpelChain > out;
  return build_chains ("subpel_batch", kStage, chains, nchains, 0, nullptr, out);
}

int
schro_hip_subpel_error_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains, int mvprec, void *const *tables)
{
  SCHRO_HIP_REQUIRE (ctx, "subpel_error_batch: bad arguments");
  std::vector < SubpelChain > out;
  int r = build_chains ("subpel_error_batch", kError, chains, nchains, mvprec, tables, out);
  if (r)
    return r;
  const int total = lay_out (out.data (), nchains);
  (void) hipSetDevice (ctx->device);
  void *dev;
  r = push_big_table (ctx, out.data (), sizeof (SubpelChain) * out.size (), &dev);
  return r ? r : launch_subpel_error (ctx->stream, (const SubpelChain *) dev, nchains, total, mvprec);
}

int
schro_hip_subpel_choose_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains, int mvprec, void *const *tables)
{
  SCHRO_HIP_REQUIRE (ctx, "subpel_choose_batch: bad arguments");
  std::vector < SubpelChain > out;
  int r = build_chains ("subpel_choose_batch", kChoose, chains, nchains, mvprec, tables, out);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);
  void *dev;
  r = push_big_table (ctx, out.data (), sizeof (SubpelChain) * out.size (), &dev);
  return r ? r : launch_subpel_choose (ctx->stream, (const SubpelChain *) dev, nchains, mvprec);
}

int
schro_hip_subpel_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains)
{
  const char *who = "subpel_batch";
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  std::vector < SubpelChain > all;
  int r = build_chains (who, kStage, chains, nchains, 0, nullptr, all);
  if (r)
    return r;
  // the tables: a slot of the queue's scratch per chain that has a pass
  int passes = 0;
  size_t need = 0;
  std::vector < size_t > slot (nchains, 0);
  for (int c = 0; c < nchains; c++) {
    passes = std::max (passes, chains[c].mv_precision);
    if (chains[c].mv_precision > 0) {
      slot[c] = need;
      need += round_up ((size_t) all[c].nbx * all[c].nby * 8 * sizeof (int32_t), 256);
    }
  }
  (void) hipSetDevice (ctx->device);
  if (need) {
    r = ensure_scratch (ctx, need);
    if (r)
      return r;
  }
  for (int c = 0; c < nchains; c++) {
    all[c].table = (int32_t *) ((uint8_t *) ctx->scratch_ref () + slot[c]);
    if (chains[c].src_field != chains[c].field)
      SCHRO_HIP_CHECK (hipMemcpyAsync (chains[c].field, chains[c].src_field, (size_t) all[c].nbx * all[c].nby * kMvBytes, hipMemcpyDeviceToDevice,
              ctx->stream));
  }
  if (!passes)
    return 0;
  // ONE device table for the launches of all passes: pass p's chains -- those whose precision reaches p -- one run after
  // the other
  std::vector < SubpelChain > runs;
  std::vector < int >first (passes + 2, 0), groups (passes + 1, 0);
  for (int p = 1; p <= passes; p++) {
    first[p] = (int) runs.size ();
    for (int c = 0; c < nchains; c++)
      if (chains[c].mv_precision >= p)
        runs.push_back (all[c]);
    groups[p] = lay_out (runs.data () + first[p], (int) runs.size () - first[p]);
  }
  first[passes + 1] = (int) runs.size ();
  void *dev;
  r = push_big_table (ctx, runs.data (), sizeof (SubpelChain) * runs.size (), &dev);
  if (r)
    return r;
  for (int p = 1; p <= passes; p++) {
    const SubpelChain *run = (const SubpelChain *) dev + first[p];
    const int n = first[p + 1] - first[p];
    r = launch_subpel_error (ctx->stream, run, n, groups[p], p);
    if (r)
      return r;
    r = launch_subpel_choose (ctx->stream, run, n, p);
    if (r)
      return r;
  }
  return 0;
}

}                               // extern "C"

namespace schro {

int
subpel_host_run (SchroHipContext * ctx, SchroHipSubpelChain * chains, int nchains)
{
  // the fields: slots of the queue's scratch IN FRONT of the tables schro_hip_subpel_batch takes from it -- so the scratch
  // is sized here for both and the batch finds it large enough
  std::vector < size_t > slot (nchains);
  std::vector < void *>host (nchains);
  size_t fields = 0, tables = 0;
  for (int c = 0; c < nchains; c++) {
    const size_t records = (size_t) std::max (chains[c].x_num_blocks, 0) * std::max (chains[c].y_num_blocks, 0);
    slot[c] = fields;
    fields += round_up (records * kMvBytes, 256);
    tables += round_up (records * 8 * sizeof (int32_t), 256);
  }
  (void) hipSetDevice (ctx->device);
  // (the tables lie at the scratch's start: the fields go behind them)
  int r = ensure_scratch (ctx, tables + fields + 256);
  if (r)
    return r;
  uint8_t *base = (uint8_t *) ctx->scratch_ref () + tables;
  for (int c = 0; c < nchains; c++) {
    host[c] = (void *) chains[c].src_field;
    chains[c].src_field = chains[c].field = base + slot[c];
  }
  // (refused before anything is copied)
  r = schro_hip_subpel_check (chains, nchains);
  if (r)
    return r;
  for (int c = 0; c < nchains; c++)
    SCHRO_HIP_CHECK (hipMemcpyAsync (chains[c].field, host[c], (size_t) chains[c].x_num_blocks * chains[c].y_num_blocks * kMvBytes,
            hipMemcpyHostToDevice, ctx->stream));
  r = schro_hip_subpel_batch (ctx, chains, nchains);
  if (r)
    return r;
  for (int c = 0; c < nchains; c++)
    SCHRO_HIP_CHECK (hipMemcpyAsync (host[c], chains[c].field, (size_t) chains[c].x_num_blocks * chains[c].y_num_blocks * kMvBytes,
            hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

}                               // namespace schro
