// plane_noarith_dec.cpp -- plane layer: core-syntax transform data in the VLC parse codes, read on the device
// (noarith_dec.hip).

#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr int64_t kNdMaxBytes = (int64_t) 1 << 29;      // bit positions of a payload are 32-bit
constexpr int64_t kNdMaxUnits = (int64_t) 1 << 28;      // chunk slots and codeblocks of a call are indexed with 32 bits

struct NdPlan {
  std::vector < NdSubband > sbs;
  std::vector < NdPicture > pics;
  int64_t chunks = 0, cbs = 0;
  int lane_x = 1, fill_x = 1;
};

struct NdRegion {
  uintptr_t at;
  size_t bytes;
  int pic;
  bool written;
  const char *what;
};

bool
nd_overlap (const void *a, size_t na, const void *b, size_t nb)
{
  const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
  return a0 < b0 + nb && b0 < a0 + na;
}

int
nd_build (const char *who, const SchroHipNoarithDecodePicture * pictures, int npictures, int bpp, NdPlan & plan)
{
  SCHRO_HIP_REQUIRE (pictures && npictures > 0 && npictures <= kMaxJobs, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "%s: bytes_per_sample must be 2 or 4", who);
  for (int p = 0; p < npictures; p++) {
    const SchroHipNoarithDecodePicture & pic = pictures[p];
    const int depth = pic.transform_depth, nsub = 1 + 3 * depth;
    SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "%s: picture %d: transform_depth %d", who, p, depth);
    for (int k = 0; k < 3; k++)
      SCHRO_HIP_REQUIRE (pic.iwt_width[k] > 0 && pic.iwt_height[k] > 0 && ((pic.iwt_width[k] | pic.iwt_height[k]) & ((1 << depth) - 1)) == 0
          && pic.iwt_width[k] < (1 << 15) && pic.iwt_height[k] < (1 << 15),
          "%s: picture %d, component %d: %d x %d must be positive multiples of %d below 32768", who, p, k, pic.iwt_width[k],
          pic.iwt_height[k], 1 << depth);
    for (int l = 0; l <= depth; l++)
      SCHRO_HIP_REQUIRE (pic.horiz_codeblocks[l] > 0 && pic.vert_codeblocks[l] > 0 && pic.horiz_codeblocks[l] < (1 << 15)
          && pic.vert_codeblocks[l] < (1 << 15), "%s: picture %d: %d x %d codeblocks at level %d (1 .. 32767)", who, p,
          pic.horiz_codeblocks[l], pic.vert_codeblocks[l], l);
    SCHRO_HIP_REQUIRE (pic.codeblock_mode_index == 0 || pic.codeblock_mode_index == 1, "%s: picture %d: codeblock_mode_index %d", who,
        p, pic.codeblock_mode_index);
    SCHRO_HIP_REQUIRE (pic.data || pic.data_bytes == 0, "%s: picture %d: data is NULL", who, p);
    SCHRO_HIP_REQUIRE ((uint64_t) pic.data_bytes < (uint64_t) kNdMaxBytes, "%s: picture %d: data_bytes %zu, bit positions are 32-bit "
        "(below 2^29)", who, p, pic.data_bytes);
    SCHRO_HIP_REQUIRE ((uintptr_t) pic.bytes_on_device % 4 == 0, "%s: picture %d: bytes_on_device is unaligned", who, p);
    SCHRO_HIP_REQUIRE (pic.result && (uintptr_t) pic.result % 4 == 0, "%s: picture %d: result is NULL or unaligned", who, p);
    SCHRO_HIP_REQUIRE (!nd_overlap (pic.result, sizeof (SchroHipNoarithDecodeResult), pic.data, pic.data_bytes), "%s: picture %d: result "
        "overlaps data", who, p);
    SCHRO_HIP_REQUIRE (!pic.bytes_on_device || !nd_overlap (pic.result, sizeof (SchroHipNoarithDecodeResult), pic.bytes_on_device, 4),
        "%s: picture %d: result overlaps bytes_on_device", who, p);
    const bool have_quant = pic.quant[0] || pic.quant[1] || pic.quant[2];
    NdPicture np;
    memset (&np, 0, sizeof (np));
    np.data = pic.data;
    np.bytes_on_device = pic.bytes_on_device;
    np.result = pic.result;
    np.data_bytes = (uint32_t) pic.data_bytes;
    np.sb_first = (int) plan.sbs.size ();
    np.nsb = 3 * nsub;
    np.mode = pic.codeblock_mode_index;
    np.is_intra = pic.is_intra != 0;
    np.compat = pic.compat_quant_offset != 0;
    for (int k = 0; k < 3; k++) {
      SCHRO_HIP_REQUIRE (pic.coeffs[k] && (uintptr_t) pic.coeffs[k] % bpp == 0, "%s: picture %d: coeffs[%d] is NULL or misaligned", who, p, k);
      SCHRO_HIP_REQUIRE (!have_quant || (pic.quant[k] && (uintptr_t) pic.quant[k] % bpp == 0), "%s: picture %d: quant[%d] is NULL or "
          "misaligned (all three or none)", who, p, k);
      SCHRO_HIP_REQUIRE ((int64_t) pic.stride[k] >= (int64_t) pic.iwt_width[k] * bpp && pic.stride[k] % bpp == 0
          && ((int64_t) pic.stride[k] << depth) < ((int64_t) 1 << 31), "%s: picture %d: stride[%d] %d for %d samples of %d bytes", who, p,
          k, pic.stride[k], pic.iwt_width[k], bpp);
      SCHRO_HIP_REQUIRE ((int64_t) (pic.iwt_height[k] - 1) * pic.stride[k] + (int64_t) pic.iwt_width[k] * bpp <= (int64_t) pic.bytes[k]
          && (uint64_t) pic.bytes[k] < ((uint64_t) 1 << 40),
          "%s: picture %d, component %d: %d rows of %d samples at stride %d reach outside the plane's %zu bytes", who, p, k,
          pic.iwt_height[k], pic.iwt_width[k], pic.stride[k], pic.bytes[k]);
      SCHRO_HIP_REQUIRE (!nd_overlap (pic.data, pic.data_bytes, pic.coeffs[k], pic.bytes[k]), "%s: picture %d: data overlaps coeffs[%d]",
          who, p, k);
      SCHRO_HIP_REQUIRE (!nd_overlap (pic.result, sizeof (SchroHipNoarithDecodeResult), pic.coeffs[k], pic.bytes[k]),
          "%s: picture %d: result overlaps coeffs[%d]", who, p, k);
      SCHRO_HIP_REQUIRE (!pic.bytes_on_device || !nd_overlap (pic.bytes_on_device, 4, pic.coeffs[k], pic.bytes[k]),
          "%s: picture %d: bytes_on_device overlaps coeffs[%d]", who, p, k);
      for (int j = 0; j < k; j++)
        SCHRO_HIP_REQUIRE (!nd_overlap (pic.coeffs[k], pic.bytes[k], pic.coeffs[j], pic.bytes[j]), "%s: picture %d: coeffs[%d] overlaps "
            "coeffs[%d]", who, p, k, j);
      if (have_quant) {
        SCHRO_HIP_REQUIRE (!nd_overlap (pic.data, pic.data_bytes, pic.quant[k], pic.bytes[k]), "%s: picture %d: data overlaps quant[%d]",
            who, p, k);
        SCHRO_HIP_REQUIRE (!nd_overlap (pic.result, sizeof (SchroHipNoarithDecodeResult), pic.quant[k], pic.bytes[k]),
            "%s: picture %d: result overlaps quant[%d]", who, p, k);
        SCHRO_HIP_REQUIRE (!pic.bytes_on_device || !nd_overlap (pic.bytes_on_device, 4, pic.quant[k], pic.bytes[k]),
            "%s: picture %d: bytes_on_device overlaps quant[%d]", who, p, k);
        for (int j = 0; j < 3; j++)
          SCHRO_HIP_REQUIRE (!nd_overlap (pic.quant[k], pic.bytes[k], pic.coeffs[j], pic.bytes[j]), "%s: picture %d: quant[%d] overlaps "
              "coeffs[%d]", who, p, k, j);
        for (int j = 0; j < k; j++)
          SCHRO_HIP_REQUIRE (!nd_overlap (pic.quant[k], pic.bytes[k], pic.quant[j], pic.bytes[j]), "%s: picture %d: quant[%d] overlaps "
              "quant[%d]", who, p, k, j);
      }
      for (int i = 0; i < nsub; i++) {
        const int position = i == 0 ? 0 : (((i - 1) / 3) << 2) | ((i - 1) % 3 + 1);
        const int level = position >> 2, shift = depth - level;     // SCHRO_SUBBAND_SHIFT
        NdSubband s;
        memset (&s, 0, sizeof (s));
        s.stride = pic.stride[k] << shift;
        s.bw = pic.iwt_width[k] >> shift;
        s.bh = pic.iwt_height[k] >> shift;
        s.hc = pic.horiz_codeblocks[i == 0 ? 0 : level + 1];
        s.vc = pic.vert_codeblocks[i == 0 ? 0 : level + 1];
        const size_t base = (size_t) ((position & 2) ? s.stride >> 1 : 0) + (size_t) ((position & 1) ? s.bw * bpp : 0);
        s.coeffs = (char *) pic.coeffs[k] + base;
        s.quant = have_quant ? (char *) pic.quant[k] + base : nullptr;
        s.cb_base = (int) plan.cbs;
        s.pic = p;
        s.comp = k;
        s.index = i;
        plan.sbs.push_back (s);
        plan.cbs += (int64_t) s.hc * s.vc;
        plan.fill_x = (int) std::min < int64_t > (kNdFillGridX, std::max < int64_t > (plan.fill_x, (int64_t) s.bh * s.hc));
      }
    }
    // a payload of b bytes takes (b + 7) / 8 chunks, and the payloads do not overlap
    np.chunk_first = (uint32_t) plan.chunks;
    np.chunk_cap = (uint32_t) (pic.data_bytes / 8 + (size_t) np.nsb + 1);
    plan.chunks += np.chunk_cap;
    plan.lane_x = std::max (plan.lane_x, (int) ((np.chunk_cap + kNdLaneThreads - 1) / kNdLaneThreads));
    SCHRO_HIP_REQUIRE (plan.chunks < kNdMaxUnits && plan.cbs < kNdMaxUnits, "%s: picture %d: more than 2^28 chunks or codeblocks in one "
        "call", who, p);
    plan.pics.push_back (np);
  }
  // what one picture writes (planes, result) may not touch what another reads or writes: the results are cleared in front of
  // the first launch, and all pictures run in every launch
  std::vector < NdRegion > regs;
  for (int p = 0; p < npictures; p++) {
    const SchroHipNoarithDecodePicture & pic = pictures[p];
    regs.push_back ({ (uintptr_t) pic.result, sizeof (SchroHipNoarithDecodeResult), p, true, "result" });
    for (int k = 0; k < 3; k++) {
      regs.push_back ({ (uintptr_t) pic.coeffs[k], pic.bytes[k], p, true, "coeffs" });
      if (pic.quant[k])
        regs.push_back ({ (uintptr_t) pic.quant[k], pic.bytes[k], p, true, "quant" });
    }
    if (pic.data_bytes)
      regs.push_back ({ (uintptr_t) pic.data, pic.data_bytes, p, false, "data" });
    if (pic.bytes_on_device)
      regs.push_back ({ (uintptr_t) pic.bytes_on_device, 4, p, false, "bytes_on_device" });
  }
  if (npictures > 1) {
    std::sort (regs.begin (), regs.end (), [](const NdRegion & a, const NdRegion & b) { return a.at < b.at; });
    // in address order: a region overlaps a later one only while that one starts in front of the furthest end seen so far
    for (size_t i = 0; i < regs.size (); i++)
      for (size_t j = i + 1; j < regs.size () && regs[j].at < regs[i].at + regs[i].bytes; j++)
        SCHRO_HIP_REQUIRE (regs[i].pic == regs[j].pic || !(regs[i].written || regs[j].written),
            "%s: picture %d: its %s overlaps the %s of picture %d", who, std::max (regs[i].pic, regs[j].pic),
            regs[i].pic > regs[j].pic ? regs[i].what : regs[j].what, regs[i].pic > regs[j].pic ? regs[j].what : regs[i].what,
            std::min (regs[i].pic, regs[j].pic));
  }
  return 0;
}

}                               // namespace

extern "C" {

int
schro_hip_noarith_decode_check (const SchroHipNoarithDecodePicture * pictures, int npictures, int bytes_per_sample)
{
  NdPlan plan;
  return nd_build ("noarith_decode_batch", pictures, npictures, bytes_per_sample, plan);
}

int64_t
schro_hip_noarith_decode_scratch_words (const SchroHipNoarithDecodePicture * pictures, int npictures, int bytes_per_sample)
{
  NdPlan plan;
  const int r = nd_build ("noarith_decode_scratch_words", pictures, npictures, bytes_per_sample, plan);
  if (r)
    return r;
  return (int64_t) nd_scratch_words ((size_t) plan.chunks, (size_t) plan.cbs, plan.sbs.size (), plan.pics.size ());
}

int
schro_hip_noarith_decode_batch (SchroHipContext * ctx, const SchroHipNoarithDecodePicture * pictures, int npictures, int bytes_per_sample)
{
  const char *who = "noarith_decode_batch";
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  NdPlan plan;
  int r = nd_build (who, pictures, npictures, bytes_per_sample, plan);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);

  // scratch of the selected queue: five words per chunk slot, three per codeblock, eight per sub-band, two per picture
  const size_t nch = (size_t) plan.chunks, nc = (size_t) plan.cbs, ns = plan.sbs.size (), npic = plan.pics.size ();
  r = ensure_scratch (ctx, nd_scratch_words (nch, nc, ns, npic) * sizeof (uint32_t));
  if (r)
    return r;
  uint32_t *w = (uint32_t *) ctx->scratch_ref ();
  NdScratch S;
  S.bands = (NdBand *) w;
  w += kNdBandWords * ns;
  S.ptotal = w;
  w += kNdPicWords * npic;
  S.sum = w;
  S.rec = w + 2 * nch;
  w += kNdChunkWords * nch;
  S.cb = w;

  // one table: the sub-bands, the pictures
  const size_t sb_bytes = ns * sizeof (NdSubband), pic_bytes = npic * sizeof (NdPicture), bytes = sb_bytes + pic_bytes;
  void *host, *dev;
  r = big_table_begin (ctx, bytes, &host, &dev);
  if (r)
    return r;
  memcpy (host, plan.sbs.data (), sb_bytes);
  memcpy ((char *) host + sb_bytes, plan.pics.data (), pic_bytes);
  r = big_table_commit (ctx, bytes);
  if (r)
    return r;
  // (A/B runs, scripts/noarith_decode_ab.py: one launch at a time on the tables the call before left)
  const char *env = SCHRO_ENV ("SCHRO_HIP_NADEC_STAGES");
  const int stages = env && atoi (env) > 0 ? atoi (env) & 15 : 15;
  if (stages & 1)
    for (int p = 0; p < npictures; p++)
      SCHRO_HIP_CHECK (hipMemsetAsync (pictures[p].result, 0, sizeof (SchroHipNoarithDecodeResult), ctx->stream));
  return launch_noarith_decode (ctx->stream, (const NdSubband *) dev, (int) ns, (const NdPicture *) ((const char *) dev + sb_bytes),
      npictures, S, bytes_per_sample, plan.lane_x, plan.fill_x, stages);
}

}                               // extern "C"
