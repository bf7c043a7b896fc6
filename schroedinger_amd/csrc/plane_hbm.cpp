// plane_hbm.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: hierarchical block matching on the
// device, the default encoder's motion search -- one level (schro_hip_hbm_level_batch), the whole chain with or without
// level 0 (schro_hip_hbm_batch), their refusals without a context (schro_hip_hbm_level_check, schro_hip_hbm_check) and
// the frame layer's run over host fields (hbm_host_run).  The kernel is hier_bm.hip.

#include "schro_hip_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr int kMaxRange = (SCHRO_HIP_LIMIT_METRIC_SCAN - 1) / 2;        // a window of 2 * h_range + 1 positions
constexpr int kMaxShift = SCHRO_HIP_MAX_HIER_LEVELS;
const char *const kField = "the field", *const kInput = "a plane or hint field";

// one level of a chain into the kernel's record, its memory into `spans`
int
add_level (const char *who, const char *what, int c, int shift, const SchroHipHbmPlane & pl, const MotionGeometry & g, int range,
    const void *hint, void *field, HbmLevel * out, std::vector < MotionSpan > &spans)
{
  SCHRO_HIP_REQUIRE (shift >= 0 && shift <= kMaxShift, "%s: %s %d level %d: the shift of a level is 0 .. %d", who, what, c, shift, kMaxShift);
  SCHRO_HIP_REQUIRE ((pl.h_shift == 0 || pl.h_shift == 1) && (pl.v_shift == 0 || pl.v_shift == 1) && pl.v_shift <= pl.h_shift,
      "%s: %s %d level %d: chroma shifts %d, %d are none of 0, 0 / 1, 0 / 1, 1", who, what, c, shift, pl.h_shift, pl.v_shift);
  for (int k = 0; k < 3; k++)
    SCHRO_HIP_REQUIRE (pl.frame[k] && pl.ref[k], "%s: %s %d level %d: component %d has a NULL pointer%s", who, what, c, shift, k,
        k ? " (the metric runs over the chroma planes too)" : "");
  SCHRO_HIP_REQUIRE (field, "%s: %s %d level %d: the field is a NULL pointer", who, what, c, shift);
  SCHRO_HIP_REQUIRE (pl.width > 0 && pl.height > 0 && pl.width <= kMaxMotionPlaneSize && pl.height <= kMaxMotionPlaneSize,
      "%s: %s %d level %d: plane size %dx%d out of range", who, what, c, shift, pl.width, pl.height);
  const int cw = (pl.width + (1 << pl.h_shift) - 1) >> pl.h_shift, chh = (pl.height + (1 << pl.v_shift) - 1) >> pl.v_shift;
  for (int k = 0; k < 3; k++)
    SCHRO_HIP_REQUIRE (pl.frame_stride[k] >= (k ? cw : pl.width) && pl.ref_stride[k] >= (k ? cw : pl.width),
        "%s: %s %d level %d: component %d has a stride shorter than a row of %d", who, what, c, shift, k, k ? cw : pl.width);
  SCHRO_HIP_REQUIRE (pl.extension >= 0 && pl.extension <= kMaxMotionExtension, "%s: %s %d level %d: extension %d out of range", who, what, c, shift,
      pl.extension);
  // schro_metric_block_sad_slow returns INT_MAX for a block outside the apron, the caller asserts when every candidate
  // does (schrohierbm.c:347): neither happens from this extension on
  SCHRO_HIP_REQUIRE (pl.extension >= std::max (g.xb, g.yb), "%s: %s %d level %d: extension %d is under the block separation %d", who, what, c,
      shift, pl.extension, std::max (g.xb, g.yb));
  SCHRO_HIP_REQUIRE (range > 0, "%s: %s %d level %d: h_range %d", who, what, c, shift, range);
  SCHRO_HIP_REQUIRE (range <= kMaxRange, "%s: %s %d level %d: h_range %d gives a window of %d positions, over the limit of %d", who, what, c,
      shift, range, 2 * range + 1, SCHRO_HIP_LIMIT_METRIC_SCAN);
  SCHRO_HIP_REQUIRE (((uintptr_t) field & 3) == 0 && ((uintptr_t) hint & 3) == 0, "%s: %s %d level %d: a field is not 4-byte aligned", who, what,
      c, shift);
  memset (out, 0, sizeof (*out));
  const size_t bytes = (size_t) g.nbx * g.nby * kMvBytes;
  for (int k = 0; k < 3; k++) {
    out->frame[k] = pl.frame[k];
    out->ref[k] = pl.ref[k];
    out->frame_stride[k] = pl.frame_stride[k];
    out->ref_stride[k] = pl.ref_stride[k];
    const size_t row = k ? cw : pl.width, rows = k ? chh : pl.height;
    spans.push_back ({(uintptr_t) pl.frame[k], (uintptr_t) pl.frame[k] + (size_t) pl.frame_stride[k] * (rows - 1) + row, false, c, shift, kInput});
    spans.push_back ({(uintptr_t) pl.ref[k], (uintptr_t) pl.ref[k] + (size_t) pl.ref_stride[k] * (rows - 1) + row, false, c, shift, kInput});
  }
  out->field = (uint8_t *) field;
  out->hint = (const uint8_t *) hint;
  out->w = pl.width;
  out->h = pl.height;
  out->hs = pl.h_shift;
  out->vs = pl.v_shift;
  out->ext = pl.extension;
  out->shift = shift;
  out->dist = range;
  spans.push_back ({(uintptr_t) field, (uintptr_t) field + bytes, true, c, shift, kField});
  return 0;
}

int
build_levels (const SchroHipHbmLevel * levels, int nlevels, std::vector < HbmChain > &chains)
{
  const char *who = "hbm_level_batch", *what = "entry";
  SCHRO_HIP_REQUIRE (levels && nlevels > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (nlevels <= kMaxJobs, "%s: at most %d entries per call", who, kMaxJobs);
  std::vector < MotionSpan > spans;
  chains.resize (nlevels);
  for (int p = 0; p < nlevels; p++) {
    const SchroHipHbmLevel & lv = levels[p];
    const MotionGeometry g = { lv.x_num_blocks, lv.y_num_blocks, lv.xbsep_luma, lv.ybsep_luma, lv.ref_index };
    int r = motion_check_geometry (who, what, p, g, SCHRO_HIP_LIMIT_BLOCK_SIZE);
    if (r)
      return r;
    HbmChain & ch = chains[p];
    memset (&ch, 0, sizeof (ch));
    ch.nbx = g.nbx, ch.nby = g.nby, ch.xb = g.xb, ch.yb = g.yb, ch.ref = g.ref;
    ch.nlevels = 1;
    r = add_level (who, what, p, lv.shift, lv.plane, g, lv.h_range, lv.hint_field, lv.field, &ch.level[0], spans);
    if (r)
      return r;
    if (lv.hint_field)
      spans.push_back ({(uintptr_t) lv.hint_field, (uintptr_t) lv.hint_field + (size_t) g.nbx * g.nby * kMvBytes, false, p, lv.shift, kInput});
  }
  return motion_check_spans (who, what, spans);
}

int
build_chains (const SchroHipHbmChain * in, int nchains, int with_level0, std::vector < HbmChain > &chains)
{
  const char *who = "hbm_batch", *what = "chain";
  SCHRO_HIP_REQUIRE (in && nchains > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (nchains <= kMaxJobs, "%s: at most %d chains per call", who, kMaxJobs);
  std::vector < MotionSpan > spans;
  chains.resize (nchains);
  for (int c = 0; c < nchains; c++) {
    const SchroHipHbmChain & src = in[c];
    const MotionGeometry g = { src.x_num_blocks, src.y_num_blocks, src.xbsep_luma, src.ybsep_luma, src.ref_index };
    int r = motion_check_geometry (who, what, c, g, SCHRO_HIP_LIMIT_BLOCK_SIZE);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (src.n_levels >= 1 && src.n_levels <= SCHRO_HIP_MAX_HIER_LEVELS, "%s: %s %d: %d levels, outside 1 .. %d", who, what, c,
        src.n_levels, SCHRO_HIP_MAX_HIER_LEVELS);
    SCHRO_HIP_REQUIRE (src.levels, "%s: %s %d has no levels", who, what, c);
    HbmChain & ch = chains[c];
    memset (&ch, 0, sizeof (ch));
    ch.nbx = g.nbx, ch.nby = g.nby, ch.xb = g.xb, ch.yb = g.yb, ch.ref = g.ref;
    const int last = with_level0 ? 0 : 1;
    ch.nlevels = src.n_levels - last + 1;
    // coarse to fine, the kernel's order; schro_hbm_scan's ranges: 20, then 10, 5, .. never under 3; level 0: 3
    int half = 20;
    for (int n = 0; n < ch.nlevels; n++, half >>= 1) {
      const int shift = src.n_levels - n;
      const SchroHipHbmPlane & pl = src.levels[shift];
      const SchroHipHbmPlane & top = src.levels[src.n_levels];
      SCHRO_HIP_REQUIRE (pl.h_shift == top.h_shift && pl.v_shift == top.v_shift,
          "%s: %s %d level %d: chroma shifts %d, %d, level %d has %d, %d", who, what, c, shift, pl.h_shift, pl.v_shift, src.n_levels, top.h_shift,
          top.v_shift);
      if (shift > last) {
        const SchroHipHbmPlane & below = src.levels[shift - 1];
        SCHRO_HIP_REQUIRE (pl.width == (below.width + 1) / 2 && pl.height == (below.height + 1) / 2,
            "%s: %s %d level %d: the plane is %dx%d, half of level %d's %dx%d is %dx%d", who, what, c, shift, pl.width, pl.height, shift - 1,
            below.width, below.height, (below.width + 1) / 2, (below.height + 1) / 2);
      }
      const int range = shift == 0 ? 3 : (n == 0 ? 20 : std::max (3, half));
      r = add_level (who, what, c, shift, pl, g, range, n == 0 ? nullptr : src.fields[shift + 1], src.fields[shift], &ch.level[n], spans);
      if (r)
        return r;
    }
  }
  return motion_check_spans (who, what, spans);
}

}                               // namespace

namespace schro {

int
hbm_host_run (SchroHipContext * ctx, const char *who, const SchroHipHbmPlane * levels, int nlevels, int shift, int h_range, int with_level0,
    const SchroHipParams * params, int ref_index, const void *hint, void *const *fields)
{
  SCHRO_HIP_REQUIRE (params->x_num_blocks > 0 && params->y_num_blocks > 0 && params->x_num_blocks <= kMaxMotionBlocks
      && params->y_num_blocks <= kMaxMotionBlocks, "%s: %d x %d blocks", who, params->x_num_blocks, params->y_num_blocks);
  const size_t bytes = (size_t) params->x_num_blocks * params->y_num_blocks * kMvBytes, slot = round_up (bytes, 256);
  (void) hipSetDevice (ctx->device);
  if (h_range > 0) {
    // one level under the caller's field: slot 0 the field, slot 1 the hint
    SCHRO_HIP_REQUIRE (fields[0], "%s: level %d has no motion field", who, shift);
    int r = ensure_scratch (ctx, slot * 2);
    if (r)
      return r;
    uint8_t *base = (uint8_t *) ctx->scratch_ref ();
    SchroHipHbmLevel lv;
    memset (&lv, 0, sizeof (lv));
    lv.plane = levels[0];
    lv.x_num_blocks = params->x_num_blocks;
    lv.y_num_blocks = params->y_num_blocks;
    lv.xbsep_luma = params->xbsep_luma;
    lv.ybsep_luma = params->ybsep_luma;
    lv.shift = shift;
    lv.h_range = h_range;
    lv.ref_index = ref_index;
    lv.hint_field = hint ? base + slot : nullptr;
    lv.field = base;
    // (refused before anything is copied)
    r = schro_hip_hbm_level_check (&lv, 1);
    if (r)
      return r;
    if (hint)
      SCHRO_HIP_CHECK (hipMemcpyAsync (base + slot, hint, bytes, hipMemcpyHostToDevice, ctx->stream));
    r = schro_hip_hbm_level_batch (ctx, &lv, 1);
    if (r)
      return r;
    SCHRO_HIP_CHECK (hipMemcpyAsync (fields[0], base, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
    return 0;
  }
  const int first = with_level0 ? 0 : 1;
  for (int k = first; k <= nlevels; k++)
    SCHRO_HIP_REQUIRE (fields[k], "%s: level %d has no motion field", who, k);
  int r = ensure_scratch (ctx, slot * (nlevels + 1));
  if (r)
    return r;
  uint8_t *base = (uint8_t *) ctx->scratch_ref ();      // slot k: level k
  SchroHipHbmChain chain;
  memset (&chain, 0, sizeof (chain));
  chain.n_levels = nlevels;
  chain.levels = levels;
  chain.x_num_blocks = params->x_num_blocks;
  chain.y_num_blocks = params->y_num_blocks;
  chain.xbsep_luma = params->xbsep_luma;
  chain.ybsep_luma = params->ybsep_luma;
  chain.ref_index = ref_index;
  for (int k = first; k <= nlevels; k++)
    chain.fields[k] = base + slot * k;
  r = schro_hip_hbm_batch (ctx, &chain, 1, with_level0);
  if (r)
    return r;
  for (int k = first; k <= nlevels; k++)
    SCHRO_HIP_CHECK (hipMemcpyAsync (fields[k], base + slot * k, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

}                               // namespace schro

extern "C" {

int
schro_hip_hbm_level_check (const SchroHipHbmLevel * levels, int nlevels)
{
  std::vector < HbmChain > chains;
  return build_levels (levels, nlevels, chains);
}

int
schro_hip_hbm_check (const SchroHipHbmChain * chains, int nchains, int with_level0)
{
  std::vector < HbmChain > out;
  return build_chains (chains, nchains, with_level0, out);
}

int
schro_hip_hbm_level_batch (SchroHipContext * ctx, const SchroHipHbmLevel * levels, int nlevels)
{
  SCHRO_HIP_REQUIRE (ctx, "hbm_level_batch: bad arguments");
  std::vector < HbmChain > chains;
  int r = build_levels (levels, nlevels, chains);
  return r ? r : run_chains (ctx, chains);
}

int
schro_hip_hbm_batch (SchroHipContext * ctx, const SchroHipHbmChain * chains, int nchains, int with_level0)
{
  SCHRO_HIP_REQUIRE (ctx, "hbm_batch: bad arguments");
  std::vector < HbmChain > out;
  int r = build_chains (chains, nchains, with_level0, out);
  return r ? r : run_chains (ctx, out);
}

}                               // extern "C"
