// plane_rough.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: the hierarchical rough motion search
// on the device -- one hint level (schro_hip_rough_hint_batch), the whole chain (schro_hip_rough_me_batch), their
// refusals without a context (schro_hip_rough_hint_check, schro_hip_rough_me_check) and the frame layer's run over host
// fields (rough_me_host_run).  The kernel is rough_hint.hip.

#include "schro_hip_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr int kMaxDistance = (SCHRO_HIP_LIMIT_METRIC_SCAN - 1) / 2;     // a window of 2 * distance + 1 positions
const char *const kField = "the field", *const kInput = "a plane or hint field";

// one level of a chain into the kernel's record, its memory into `spans`
int
add_level (const char *who, const char *what, int c, int shift, const SchroHipRoughPlane & pl, const MotionGeometry & g, int dist,
    const void *hint, void *field, RoughLevel * out, std::vector < MotionSpan > &spans)
{
  SCHRO_HIP_REQUIRE (pl.frame && pl.ref && field, "%s: %s %d level %d has a NULL pointer", who, what, c, shift);
  SCHRO_HIP_REQUIRE (pl.width > 0 && pl.height > 0 && pl.width <= kMaxMotionPlaneSize && pl.height <= kMaxMotionPlaneSize,
      "%s: %s %d level %d: plane size %dx%d out of range", who, what, c, shift, pl.width, pl.height);
  SCHRO_HIP_REQUIRE (pl.frame_stride >= pl.width && pl.ref_stride >= pl.width, "%s: %s %d level %d: a stride shorter than a row", who, what, c,
      shift);
  SCHRO_HIP_REQUIRE (pl.extension >= 0 && pl.extension <= kMaxMotionExtension, "%s: %s %d level %d: extension %d out of range", who, what, c, shift,
      pl.extension);
  SCHRO_HIP_REQUIRE (dist > 0, "%s: %s %d level %d: distance %d", who, what, c, shift, dist);
  SCHRO_HIP_REQUIRE (dist <= kMaxDistance, "%s: %s %d level %d: distance %d gives a window of %d positions, over the limit of %d", who, what, c,
      shift, dist, 2 * dist + 1, SCHRO_HIP_LIMIT_METRIC_SCAN);
  SCHRO_HIP_REQUIRE (((uintptr_t) field & 3) == 0 && ((uintptr_t) hint & 3) == 0, "%s: %s %d level %d: a field is not 4-byte aligned", who, what,
      c, shift);
  memset (out, 0, sizeof (*out));
  out->frame = pl.frame;
  out->ref = pl.ref;
  out->field = (uint8_t *) field;
  out->hint = (const uint8_t *) hint;
  out->frame_stride = pl.frame_stride;
  out->ref_stride = pl.ref_stride;
  out->w = pl.width;
  out->h = pl.height;
  out->ext = pl.extension;
  out->shift = shift;
  out->dist = dist;
  const size_t plane = (size_t) pl.width, bytes = (size_t) g.nbx * g.nby * kMvBytes;
  spans.push_back ({(uintptr_t) pl.frame, (uintptr_t) pl.frame + (size_t) pl.frame_stride * (pl.height - 1) + plane, false, c, shift, kInput});
  spans.push_back ({(uintptr_t) pl.ref, (uintptr_t) pl.ref + (size_t) pl.ref_stride * (pl.height - 1) + plane, false, c, shift, kInput});
  spans.push_back ({(uintptr_t) field, (uintptr_t) field + bytes, true, c, shift, kField});
  return 0;
}

int
build_hint (const SchroHipRoughHintPicture * pictures, int npictures, std::vector < RoughChain > &chains)
{
  const char *who = "rough_hint_batch", *what = "picture";
  SCHRO_HIP_REQUIRE (pictures && npictures > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (npictures <= kMaxJobs, "%s: at most %d pictures per call", who, kMaxJobs);
  std::vector < MotionSpan > spans;
  chains.resize (npictures);
  for (int p = 0; p < npictures; p++) {
    const SchroHipRoughHintPicture & pic = pictures[p];
    const MotionGeometry g = { pic.x_num_blocks, pic.y_num_blocks, pic.xbsep_luma, pic.ybsep_luma, pic.ref_index };
    int r = motion_check_geometry (who, what, p, g, SCHRO_HIP_LIMIT_BLOCK_SIZE);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (pic.shift >= 1 && pic.shift <= SCHRO_HIP_MAX_HIER_LEVELS - 1, "%s: %s %d level %d: the shift of a hint level is 1 .. %d", who,
        what, p, pic.shift, SCHRO_HIP_MAX_HIER_LEVELS - 1);
    SCHRO_HIP_REQUIRE (pic.hint_field, "%s: %s %d level %d has no hint field", who, what, p, pic.shift);
    RoughChain & ch = chains[p];
    memset (&ch, 0, sizeof (ch));
    ch.nbx = g.nbx, ch.nby = g.nby, ch.xb = g.xb, ch.yb = g.yb, ch.ref = g.ref;
    ch.nlevels = 1;
    const SchroHipRoughPlane pl = { pic.frame, pic.frame_stride, pic.ref, pic.ref_stride, pic.width, pic.height,
      pic.extension
    };
    r = add_level (who, what, p, pic.shift, pl, g, pic.distance, pic.hint_field, pic.field, &ch.level[0], spans);
    if (r)
      return r;
    spans.push_back ({(uintptr_t) pic.hint_field, (uintptr_t) pic.hint_field + (size_t) g.nbx * g.nby * kMvBytes, false, p, pic.shift, kInput});
  }
  return motion_check_spans (who, what, spans);
}

int
build_chains (const SchroHipRoughChain * in, int nchains, int nohint_distance, int hint_distance, std::vector < RoughChain > &chains)
{
  const char *who = "rough_me_batch", *what = "chain";
  SCHRO_HIP_REQUIRE (in && nchains > 0, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (nchains <= kMaxJobs, "%s: at most %d chains per call", who, kMaxJobs);
  std::vector < MotionSpan > spans;
  chains.resize (nchains);
  for (int c = 0; c < nchains; c++) {
    const SchroHipRoughChain & src = in[c];
    const MotionGeometry g = { src.x_num_blocks, src.y_num_blocks, src.xbsep_luma, src.ybsep_luma, src.ref_index };
    int r = motion_check_geometry (who, what, c, g, SCHRO_HIP_LIMIT_BLOCK_SIZE);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (src.n_levels >= 1 && src.n_levels <= SCHRO_HIP_MAX_HIER_LEVELS, "%s: %s %d: %d levels, outside 1 .. %d", who, what, c,
        src.n_levels, SCHRO_HIP_MAX_HIER_LEVELS);
    SCHRO_HIP_REQUIRE (src.levels, "%s: %s %d has no levels", who, what, c);
    RoughChain & ch = chains[c];
    memset (&ch, 0, sizeof (ch));
    ch.nbx = g.nbx, ch.nby = g.nby, ch.xb = g.xb, ch.yb = g.yb, ch.ref = g.ref;
    ch.nlevels = src.n_levels;
    // coarse to fine: the kernel's order
    for (int n = 0; n < src.n_levels; n++) {
      const int shift = src.n_levels - n;
      const SchroHipRoughPlane & pl = src.levels[shift - 1];
      if (shift > 1) {
        const SchroHipRoughPlane & below = src.levels[shift - 2];
        SCHRO_HIP_REQUIRE (pl.width == (below.width + 1) / 2 && pl.height == (below.height + 1) / 2,
            "%s: %s %d level %d: the plane is %dx%d, half of level %d's %dx%d is %dx%d", who, what, c, shift, pl.width, pl.height, shift - 1,
            below.width, below.height, (below.width + 1) / 2, (below.height + 1) / 2);
      }
      r = add_level (who, what, c, shift, pl, g, n == 0 ? nohint_distance : hint_distance, n == 0 ? nullptr : src.fields[shift],
          src.fields[shift - 1], &ch.level[n], spans);
      if (r)
        return r;
    }
  }
  return motion_check_spans (who, what, spans);
}

}                               // namespace

namespace schro {

int
rough_me_host_run (SchroHipContext * ctx, const char *who, const SchroHipRoughPlane * levels, int nlevels, int first_shift,
    const SchroHipParams * params, int ref_index, int nohint_distance, int hint_distance, const void *hint, void *const *fields)
{
  SCHRO_HIP_REQUIRE (params->x_num_blocks > 0 && params->y_num_blocks > 0 && params->x_num_blocks <= kMaxMotionBlocks
      && params->y_num_blocks <= kMaxMotionBlocks, "%s: %d x %d blocks", who, params->x_num_blocks, params->y_num_blocks);
  for (int k = 0; k < nlevels; k++)
    SCHRO_HIP_REQUIRE (fields[k], "%s: level %d has no motion field", who, first_shift + k);
  const size_t bytes = (size_t) params->x_num_blocks * params->y_num_blocks * kMvBytes, slot = round_up (bytes, 256);
  (void) hipSetDevice (ctx->device);
  int r = ensure_scratch (ctx, slot * (nlevels + 1));
  if (r)
    return r;
  uint8_t *base = (uint8_t *) ctx->scratch_ref ();      // slot k: level first_shift + k; slot nlevels: the hint
  if (hint) {
    // one hint level under the caller's field
    SchroHipRoughHintPicture pic;
    memset (&pic, 0, sizeof (pic));
    pic.frame = levels[0].frame;
    pic.frame_stride = levels[0].frame_stride;
    pic.ref = levels[0].ref;
    pic.ref_stride = levels[0].ref_stride;
    pic.width = levels[0].width;
    pic.height = levels[0].height;
    pic.extension = levels[0].extension;
    pic.x_num_blocks = params->x_num_blocks;
    pic.y_num_blocks = params->y_num_blocks;
    pic.xbsep_luma = params->xbsep_luma;
    pic.ybsep_luma = params->ybsep_luma;
    pic.shift = first_shift;
    pic.distance = hint_distance;
    pic.ref_index = ref_index;
    pic.hint_field = base + slot;
    pic.field = base;
    // (refused before anything is copied)
    r = schro_hip_rough_hint_check (&pic, 1);
    if (r)
      return r;
    SCHRO_HIP_CHECK (hipMemcpyAsync (base + slot, hint, bytes, hipMemcpyHostToDevice, ctx->stream));
    r = schro_hip_rough_hint_batch (ctx, &pic, 1);
    if (r)
      return r;
    SCHRO_HIP_CHECK (hipMemcpyAsync (fields[0], base, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
    return 0;
  }
  SchroHipRoughChain chain;
  memset (&chain, 0, sizeof (chain));
  chain.n_levels = nlevels;
  chain.levels = levels;
  chain.x_num_blocks = params->x_num_blocks;
  chain.y_num_blocks = params->y_num_blocks;
  chain.xbsep_luma = params->xbsep_luma;
  chain.ybsep_luma = params->ybsep_luma;
  chain.ref_index = ref_index;
  for (int k = 0; k < nlevels; k++)
    chain.fields[k] = base + slot * k;
  r = schro_hip_rough_me_batch (ctx, &chain, 1, nohint_distance, hint_distance);
  if (r)
    return r;
  for (int k = 0; k < nlevels; k++)
    SCHRO_HIP_CHECK (hipMemcpyAsync (fields[k], base + slot * k, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

}                               // namespace schro

extern "C" {

int
schro_hip_rough_hint_check (const SchroHipRoughHintPicture * pictures, int npictures)
{
  std::vector < RoughChain > chains;
  return build_hint (pictures, npictures, chains);
}

int
schro_hip_rough_me_check (const SchroHipRoughChain * chains, int nchains, int nohint_distance, int hint_distance)
{
  std::vector < RoughChain > out;
  return build_chains (chains, nchains, nohint_distance, hint_distance, out);
}

int
schro_hip_rough_hint_batch (SchroHipContext * ctx, const SchroHipRoughHintPicture * pictures, int npictures)
{
  SCHRO_HIP_REQUIRE (ctx, "rough_hint_batch: bad arguments");
  std::vector < RoughChain > chains;
  int r = build_hint (pictures, npictures, chains);
  return r ? r : run_chains (ctx, chains);
}

int
schro_hip_rough_me_batch (SchroHipContext * ctx, const SchroHipRoughChain * chains, int nchains, int nohint_distance, int hint_distance)
{
  SCHRO_HIP_REQUIRE (ctx, "rough_me_batch: bad arguments");
  std::vector < RoughChain > out;
  int r = build_chains (chains, nchains, nohint_distance, hint_distance, out);
  return r ? r : run_chains (ctx, out);
}

}                               // extern "C"
