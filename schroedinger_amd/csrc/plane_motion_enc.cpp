// plane_motion_enc.cpp -- plane layer: the motion data of a noarith (VLC) picture, written on the device (motion_enc.hip).

#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr int64_t kMeMaxBound = (int64_t) 1 << 29;      // bit positions are 32-bit

int
me_check_geometry (const char *who, int p, int nbx, int nby, int num_refs)
{
  SCHRO_HIP_REQUIRE (nbx > 0 && nby > 0 && nbx % 4 == 0 && nby % 4 == 0 && nbx <= kMaxMotionBlocks && nby <= kMaxMotionBlocks,
      "%s: picture %d: %d x %d blocks must be positive multiples of 4, at most %d", who, p, nbx, nby, kMaxMotionBlocks);
  SCHRO_HIP_REQUIRE (num_refs == 1 || num_refs == 2, "%s: picture %d: num_refs %d (1 or 2)", who, p, num_refs);
  return 0;
}

// A vector or DC difference of two int16 codes in at most 34 bits (magnitude <= 65535: 2 * 17 - 1 bits of uint code and
// the sign).  A block carries either its vectors -- x and y per reference: 4 codes with two references, 2 with one -- or
// three DCs: 136 bits with two references, 102 with one.  Its mode takes one bit per reference and one more with global
// motion; a superblock's split residual is 0 .. 2: at most 3 bits.  The payloads of the 7 or 9 sections together take
// these bits and less than one byte of padding each; a section's length code is uint (length < 2^29), at most 59 bits,
// 8 bytes with its padding.  So 9 bytes per section on top of the bits.
int64_t
me_bound (int nbx, int nby, int num_refs, int have_global)
{
  const int64_t blocks = (int64_t) nbx * nby, sections = num_refs > 1 ? 9 : 7;
  const int64_t per_block = (num_refs > 1 ? 136 : 102) + 1 + (num_refs > 1 ? 1 : 0) + (have_global ? 1 : 0);
  return (blocks * per_block + blocks / 16 * 3 + 7) / 8 + 9 * sections;
}

struct MePlan {
  std::vector < MePicture > pics;
  int64_t sbs = 0;
  int waves_x = 1, clear_x = 1;
};

int
me_build (const char *who, const SchroHipMotionEncodePicture * pictures, int npictures, MePlan & plan)
{
  SCHRO_HIP_REQUIRE (pictures && npictures > 0 && npictures <= kMaxJobs, "%s: bad arguments", who);
  std::vector < MotionSpan > spans;
  for (int p = 0; p < npictures; p++) {
    const SchroHipMotionEncodePicture & pic = pictures[p];
    int r = me_check_geometry (who, p, pic.x_num_blocks, pic.y_num_blocks, pic.num_refs);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (pic.motion && (uintptr_t) pic.motion % 4 == 0, "%s: picture %d: motion is NULL or not 4-byte aligned", who, p);
    SCHRO_HIP_REQUIRE (pic.out, "%s: picture %d: out is NULL", who, p);
    SCHRO_HIP_REQUIRE (pic.result && (uintptr_t) pic.result % 4 == 0, "%s: picture %d: result is NULL or not 4-byte aligned", who, p);
    const int64_t bound = me_bound (pic.x_num_blocks, pic.y_num_blocks, pic.num_refs, pic.have_global_motion);
    SCHRO_HIP_REQUIRE (bound < kMeMaxBound, "%s: picture %d: a bound of %lld bytes, bit positions are 32-bit (below 2^29)", who, p,
        (long long) bound);
    const size_t records = (size_t) pic.x_num_blocks * pic.y_num_blocks;
    const size_t most = (size_t) std::min < uint64_t > (pic.capacity, (uint64_t) bound);
    spans.push_back ({(uintptr_t) pic.motion, (uintptr_t) pic.motion + records * kMvBytes, false, p, -1, "the field"});
    spans.push_back ({(uintptr_t) pic.out, (uintptr_t) pic.out + most, true, p, -1, "out"});
    spans.push_back ({(uintptr_t) pic.result, (uintptr_t) pic.result + sizeof (SchroHipMotionEncodeResult), true, p, -1, "the result"});
    MePicture mp;
    memset (&mp, 0, sizeof (mp));
    mp.motion = (const uint8_t *) pic.motion;
    mp.out = pic.out;
    mp.result = pic.result;
    mp.capacity = (uint32_t) std::min < uint64_t > (pic.capacity, (uint64_t) kMeMaxBound);
    mp.nbx = pic.x_num_blocks;
    mp.nby = pic.y_num_blocks;
    mp.num_refs = pic.num_refs;
    mp.have_global = pic.have_global_motion ? 1 : 0;
    mp.sb_first = (int) plan.sbs;
    plan.pics.push_back (mp);
    const int64_t nsb = (int64_t) records / 16;
    plan.sbs += nsb;
    SCHRO_HIP_REQUIRE (plan.sbs * kMeSbWords < ((int64_t) 1 << 31), "%s: picture %d: more than 2^26 superblocks in one call", who, p);
    plan.waves_x = (int) std::max < int64_t > (plan.waves_x, (nsb + 3) / 4);
    // the clear launch: 4 KiB of output per workgroup, over the most a picture can take
    plan.clear_x = (int) std::max < int64_t > (plan.clear_x, ((int64_t) most + 3 + 4095) / 4096);
  }
  return motion_check_spans (who, "picture", spans);
}

}                               // namespace

extern "C" {

int64_t
schro_hip_motion_encode_bound (int x_num_blocks, int y_num_blocks, int num_refs, int have_global_motion)
{
  int r = me_check_geometry ("motion_encode_bound", 0, x_num_blocks, y_num_blocks, num_refs);
  if (r)
    return r;
  return me_bound (x_num_blocks, y_num_blocks, num_refs, have_global_motion);
}

int
schro_hip_motion_encode_check (const SchroHipMotionEncodePicture * pictures, int npictures)
{
  MePlan plan;
  return me_build ("motion_encode_batch", pictures, npictures, plan);
}

int
schro_hip_motion_encode_batch (SchroHipContext * ctx, const SchroHipMotionEncodePicture * pictures, int npictures)
{
  const char *who = "motion_encode_batch";
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  MePlan plan;
  int r = me_build (who, pictures, npictures, plan);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);

  // scratch of the selected queue: kMeSbWords words per superblock, the sections' header bits and lengths per picture
  const size_t np = plan.pics.size ();
  r = ensure_scratch (ctx, ((size_t) plan.sbs * kMeSbWords + np * 2 * kMeSections) * sizeof (uint32_t));
  if (r)
    return r;
  uint32_t *scratch = (uint32_t *) ctx->scratch_ref ();
  const size_t bytes = np * sizeof (MePicture);
  void *host, *dev;
  r = big_table_begin (ctx, bytes, &host, &dev);
  if (r)
    return r;
  memcpy (host, plan.pics.data (), bytes);
  r = big_table_commit (ctx, bytes);
  if (r)
    return r;
  // (A/B runs, scripts/motion_encode_ab.py: one launch at a time on the tables the call before left)
  const char *env = SCHRO_ENV ("SCHRO_HIP_MOTENC_STAGES");
  const int stages = env && atoi (env) > 0 ? atoi (env) & 15 : 15;
  // (the layout launch writes every word of every result: nothing to clear first)
  return launch_motion_encode (ctx->stream, (const MePicture *) dev, npictures, scratch, (int) plan.sbs, plan.waves_x, plan.clear_x, stages);
}

}                               // extern "C"
