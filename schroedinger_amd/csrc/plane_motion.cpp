// plane_motion.cpp -- what the plane layers of the encoder's motion stages share on the host (plane_rough.cpp,
// plane_hbm.cpp, plane_subpel.cpp, plane_split2.cpp, plane_mode.cpp): the refusals of a block grid and of a picture under
// an upsampled reference, the overlap check over the device memory a call reads and writes, and the launch of a batch of
// chains.  Every refusal's text exists here once; what a stage refuses alone stays in its own file, in its own order.

#include "schro_hip_internal.h"

#include <cmath>
#include <algorithm>

namespace schro {

int
motion_check_blocks (const char *who, const char *what, int c, int nbx, int nby)
{
  SCHRO_HIP_REQUIRE (nbx > 0 && nby > 0 && nbx <= kMaxMotionBlocks && nby <= kMaxMotionBlocks, "%s: %s %d: %d x %d blocks", who, what, c, nbx, nby);
  return 0;
}

int
motion_check_block_size (const char *who, const char *what, int c, int xb, int yb, int max_block)
{
  SCHRO_HIP_REQUIRE (xb > 0 && yb > 0 && xb <= max_block && yb <= max_block, "%s: %s %d: a block of %d x %d is outside 1 .. %d", who, what, c, xb, yb,
      max_block);
  return 0;
}

int
motion_check_geometry (const char *who, const char *what, int c, const MotionGeometry & g, int max_block)
{
  int r = motion_check_blocks (who, what, c, g.nbx, g.nby);
  if (!r)
    r = motion_check_block_size (who, what, c, g.xb, g.yb, max_block);
  if (r)
    return r;
  SCHRO_HIP_REQUIRE (g.ref == 0 || g.ref == 1, "%s: %s %d: reference %d is neither 0 nor 1", who, what, c, g.ref);
  return 0;
}

int
motion_check_precision (const char *who, const char *what, int c, int mv_precision)
{
  SCHRO_HIP_REQUIRE (mv_precision >= 0 && mv_precision <= 3, "%s: %s %d: mv_precision %d is outside 0 .. 3", who, what, c, mv_precision);
  return 0;
}

int
motion_check_picture (const char *who, const char *what, int c, int width, int height, int xb, int yb, int extension, int mv_precision, double lambda)
{
  SCHRO_HIP_REQUIRE (width > 0 && height > 0 && width <= kMaxVector && height <= kMaxVector, "%s: %s %d: picture size %dx%d out of range", who, what, c,
      width, height);
  const int block = std::max (xb, yb);
  SCHRO_HIP_REQUIRE (extension >= block, "%s: %s %d: extension %d is under the block separation %d", who, what, c, extension, block);
  SCHRO_HIP_REQUIRE (extension <= kMaxTiledExtension, "%s: %s %d: extension %d is over the %d apron columns of an upsampled image", who, what, c,
      extension, kMaxTiledExtension);
  const int reach = (std::max (width, height) << mv_precision) + extension;
  SCHRO_HIP_REQUIRE (reach <= kMaxVector, "%s: %s %d: %dx%d at mv_precision %d: a coordinate of %d does not fit a vector of 16 bits", who, what, c, width,
      height, mv_precision, reach);
  SCHRO_HIP_REQUIRE (std::isfinite (lambda) && lambda >= 0, "%s: %s %d: lambda %g is negative or not finite", who, what, c, lambda);
  return 0;
}

int
motion_check_spans (const char *who, const char *what, std::vector < MotionSpan > &spans)
{
  std::sort (spans.begin (), spans.end (), [](const MotionSpan & a, const MotionSpan & b) {
        return a.begin < b.begin;}
  );
  const MotionSpan *any = nullptr, *written = nullptr;  // the spans seen so far that end last
  for (const MotionSpan & s:spans) {
    const MotionSpan *hit = s.written ? any : written;
    if (hit && hit->end > s.begin) {
      if (s.level < 0)
        return set_error (SCHRO_HIP_EINVAL, "%s: %s %d: %s overlaps %s of %s %d", who, what, s.owner, s.name, hit->name, what, hit->owner);
      return set_error (SCHRO_HIP_EINVAL, "%s: %s %d level %d: %s overlaps %s of %s %d level %d", who, what, s.owner, s.level, s.name, hit->name, what,
          hit->owner, hit->level);
    }
    if (!any || s.end > any->end)
      any = &s;
    if (s.written && (!written || s.end > written->end))
      written = &s;
  }
  return 0;
}

namespace {

// the table to the device and the launch: as much LDS per wave as the largest block and window of any level need
template < class Chain, class Launch > int
run (SchroHipContext * ctx, const std::vector < Chain > &chains, Launch launch)
{
  size_t lds = 0;
  for (const Chain & ch:chains)
    for (int n = 0; n < ch.nlevels; n++) {
      const int span = 2 * ch.level[n].dist + 1;
      lds = std::max (lds, scan_lds_bytes (ch.xb, ch.yb, span, span));
    }
  (void) hipSetDevice (ctx->device);
  void *dev;
  int r = push_big_table (ctx, chains.data (), sizeof (Chain) * chains.size (), &dev);
  if (r)
    return r;
  return launch (ctx->stream, (const Chain *) dev, (int) chains.size (), lds);
}

}                               // namespace

int
run_chains (SchroHipContext * ctx, const std::vector < RoughChain > &chains)
{
  return run (ctx, chains, launch_rough_hint);
}

int
run_chains (SchroHipContext * ctx, const std::vector < HbmChain > &chains)
{
  return run (ctx, chains, launch_hier_bm);
}

}                               // namespace schro
