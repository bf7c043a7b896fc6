// plane_motion_arith_dec.cpp -- plane layer: the motion data of an arithmetic-coded picture, read on the device
// (motion_arith_dec.hip).  The refusals are plane_motion_dec.cpp's, in the same words.

#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>

using namespace schro;

namespace {

constexpr uint64_t kMaMaxBytes = (uint64_t) 1 << 29;    // as the VLC call: positions in a picture's bytes are 32-bit

struct MaPlan {
  std::vector < MaPicture > pics;
  uint64_t words = 0;
};

int
ma_build (const char *who, const SchroHipMotionArithDecodePicture * pictures, int npictures, MaPlan & plan)
{
  SCHRO_HIP_REQUIRE (pictures && npictures > 0 && npictures <= kMaxJobs, "%s: bad arguments", who);
  std::vector < MotionSpan > spans;
  for (int p = 0; p < npictures; p++) {
    const SchroHipMotionArithDecodePicture & pic = pictures[p];
    const int nbx = pic.x_num_blocks, nby = pic.y_num_blocks;
    SCHRO_HIP_REQUIRE (nbx > 0 && nby > 0 && nbx % 4 == 0 && nby % 4 == 0 && nbx <= kMaxMotionBlocks && nby <= kMaxMotionBlocks,
        "%s: picture %d: %d x %d blocks must be positive multiples of 4, at most %d", who, p, nbx, nby, kMaxMotionBlocks);
    SCHRO_HIP_REQUIRE (pic.num_refs == 1 || pic.num_refs == 2, "%s: picture %d: num_refs %d (1 or 2)", who, p, pic.num_refs);
    SCHRO_HIP_REQUIRE (pic.data, "%s: picture %d: data is NULL", who, p);
    SCHRO_HIP_REQUIRE (pic.motion && (uintptr_t) pic.motion % 4 == 0, "%s: picture %d: motion is NULL or not 4-byte aligned", who, p);
    SCHRO_HIP_REQUIRE (pic.result && (uintptr_t) pic.result % 4 == 0, "%s: picture %d: result is NULL or not 4-byte aligned", who, p);
    SCHRO_HIP_REQUIRE ((uintptr_t) pic.bytes_on_device % 4 == 0, "%s: picture %d: bytes_on_device is not 4-byte aligned", who, p);
    SCHRO_HIP_REQUIRE ((uint64_t) pic.data_bytes < kMaMaxBytes, "%s: picture %d: data_bytes %zu, bit positions are 32-bit (below 2^29)", who, p,
        pic.data_bytes);
    const size_t records = (size_t) nbx * nby;
    if (pic.data_bytes)
      spans.push_back ({(uintptr_t) pic.data, (uintptr_t) pic.data + pic.data_bytes, false, p, -1, "data"});
    if (pic.bytes_on_device)
      spans.push_back ({(uintptr_t) pic.bytes_on_device, (uintptr_t) pic.bytes_on_device + 4, false, p, -1, "bytes_on_device"});
    spans.push_back ({(uintptr_t) pic.motion, (uintptr_t) pic.motion + records * kMvBytes, true, p, -1, "the field"});
    spans.push_back ({(uintptr_t) pic.result, (uintptr_t) pic.result + sizeof (SchroHipMotionArithDecodeResult), true, p, -1, "the result"});
    MaPicture mp;
    memset (&mp, 0, sizeof (mp));
    mp.data = pic.data;
    mp.bytes_on_device = pic.bytes_on_device;
    mp.motion = (uint8_t *) pic.motion;
    mp.result = pic.result;
    mp.scratch_first = plan.words;
    mp.data_bytes = (uint32_t) pic.data_bytes;
    mp.nbx = nbx;
    mp.nby = nby;
    mp.num_refs = pic.num_refs;
    mp.have_global = pic.have_global_motion ? 1 : 0;
    plan.pics.push_back (mp);
    plan.words += ma_picture_words (records);
  }
  return motion_check_spans (who, "picture", spans);
}

}                               // namespace

extern "C" {

int
schro_hip_motion_arith_decode_check (const SchroHipMotionArithDecodePicture * pictures, int npictures)
{
  MaPlan plan;
  return ma_build ("motion_arith_decode_batch", pictures, npictures, plan);
}

int64_t
schro_hip_motion_arith_decode_scratch_words (const SchroHipMotionArithDecodePicture * pictures, int npictures)
{
  MaPlan plan;
  int r = ma_build ("motion_arith_decode_scratch_words", pictures, npictures, plan);
  return r ? r : (int64_t) plan.words;
}

int
schro_hip_motion_arith_decode_batch (SchroHipContext * ctx, const SchroHipMotionArithDecodePicture * pictures, int npictures)
{
  const char *who = "motion_arith_decode_batch";
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  MaPlan plan;
  int r = ma_build (who, pictures, npictures, plan);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);
  r = ensure_scratch (ctx, (size_t) plan.words * sizeof (uint32_t));
  if (r)
    return r;
  uint32_t *scratch = (uint32_t *) ctx->scratch_ref ();
  const size_t bytes = plan.pics.size () * sizeof (MaPicture);
  void *host, *dev;
  r = big_table_begin (ctx, bytes, &host, &dev);
  if (r)
    return r;
  memcpy (host, plan.pics.data (), bytes);
  r = big_table_commit (ctx, bytes);
  if (r)
    return r;
  // (A/B runs, scripts/motion_arith_decode_ab.py: one launch at a time on the tables the call before left)
  const char *env = SCHRO_ENV ("SCHRO_HIP_MOTARITH_STAGES");
  const int stages = env && atoi (env) > 0 ? atoi (env) & 127 : 127;
  return launch_motion_arith_decode (ctx->stream, (const MaPicture *) dev, npictures, scratch, stages);
}

}                               // extern "C"
