// plane_arith_dec.cpp -- plane layer: arithmetic-coded core-syntax transform data, read on the device (arith_dec.hip).
// The refusals are those of plane_noarith_dec.cpp, stated again here for the arithmetic picture and result types so that
// the VLC path stays as it is.

#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr int64_t kAdMaxBytes = (int64_t) 1 << 29;      // as the VLC call: header positions are bit positions

struct AdPlan {
  std::vector < NdSubband > sbs;
  std::vector < AdPicture > pics;
  std::vector < AdTower > towers;
};

struct AdRegion {
  uintptr_t at;
  size_t bytes;
  int pic;
  bool written;
  const char *what;
};

bool
ad_overlap (const void *a, size_t na, const void *b, size_t nb)
{
  const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
  return a0 < b0 + nb && b0 < a0 + na;
}

int
ad_build (const char *who, const SchroHipArithDecodePicture * pictures, int npictures, int bpp, AdPlan & plan)
{
  SCHRO_HIP_REQUIRE (pictures && npictures > 0 && npictures <= kMaxJobs, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "%s: bytes_per_sample must be 2 or 4", who);
  std::vector < int64_t > work;   // samples per tower
  for (int p = 0; p < npictures; p++) {
    const SchroHipArithDecodePicture & pic = pictures[p];
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
    SCHRO_HIP_REQUIRE ((uint64_t) pic.data_bytes < (uint64_t) kAdMaxBytes, "%s: picture %d: data_bytes %zu, bit positions are 32-bit "
        "(below 2^29)", who, p, pic.data_bytes);
    SCHRO_HIP_REQUIRE ((uintptr_t) pic.bytes_on_device % 4 == 0, "%s: picture %d: bytes_on_device is unaligned", who, p);
    SCHRO_HIP_REQUIRE (pic.result && (uintptr_t) pic.result % 4 == 0, "%s: picture %d: result is NULL or unaligned", who, p);
    SCHRO_HIP_REQUIRE (!ad_overlap (pic.result, sizeof (SchroHipArithDecodeResult), pic.data, pic.data_bytes), "%s: picture %d: result "
        "overlaps data", who, p);
    SCHRO_HIP_REQUIRE (!pic.bytes_on_device || !ad_overlap (pic.result, sizeof (SchroHipArithDecodeResult), pic.bytes_on_device, 4),
        "%s: picture %d: result overlaps bytes_on_device", who, p);
    const bool have_quant = pic.quant[0] || pic.quant[1] || pic.quant[2];
    AdPicture ap;
    memset (&ap, 0, sizeof (ap));
    ap.data = pic.data;
    ap.bytes_on_device = pic.bytes_on_device;
    ap.result = pic.result;
    ap.data_bytes = (uint32_t) pic.data_bytes;
    ap.sb_first = (int) plan.sbs.size ();
    ap.nsb = 3 * nsub;
    ap.mode = pic.codeblock_mode_index;
    ap.is_intra = pic.is_intra != 0;
    ap.compat = pic.compat_quant_offset != 0;
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
      SCHRO_HIP_REQUIRE (!ad_overlap (pic.data, pic.data_bytes, pic.coeffs[k], pic.bytes[k]), "%s: picture %d: data overlaps coeffs[%d]",
          who, p, k);
      SCHRO_HIP_REQUIRE (!ad_overlap (pic.result, sizeof (SchroHipArithDecodeResult), pic.coeffs[k], pic.bytes[k]),
          "%s: picture %d: result overlaps coeffs[%d]", who, p, k);
      SCHRO_HIP_REQUIRE (!pic.bytes_on_device || !ad_overlap (pic.bytes_on_device, 4, pic.coeffs[k], pic.bytes[k]),
          "%s: picture %d: bytes_on_device overlaps coeffs[%d]", who, p, k);
      for (int j = 0; j < k; j++)
        SCHRO_HIP_REQUIRE (!ad_overlap (pic.coeffs[k], pic.bytes[k], pic.coeffs[j], pic.bytes[j]), "%s: picture %d: coeffs[%d] overlaps "
            "coeffs[%d]", who, p, k, j);
      if (have_quant) {
        SCHRO_HIP_REQUIRE (!ad_overlap (pic.data, pic.data_bytes, pic.quant[k], pic.bytes[k]), "%s: picture %d: data overlaps quant[%d]",
            who, p, k);
        SCHRO_HIP_REQUIRE (!ad_overlap (pic.result, sizeof (SchroHipArithDecodeResult), pic.quant[k], pic.bytes[k]),
            "%s: picture %d: result overlaps quant[%d]", who, p, k);
        SCHRO_HIP_REQUIRE (!pic.bytes_on_device || !ad_overlap (pic.bytes_on_device, 4, pic.quant[k], pic.bytes[k]),
            "%s: picture %d: bytes_on_device overlaps quant[%d]", who, p, k);
        for (int j = 0; j < 3; j++)
          SCHRO_HIP_REQUIRE (!ad_overlap (pic.quant[k], pic.bytes[k], pic.coeffs[j], pic.bytes[j]), "%s: picture %d: quant[%d] overlaps "
              "coeffs[%d]", who, p, k, j);
        for (int j = 0; j < k; j++)
          SCHRO_HIP_REQUIRE (!ad_overlap (pic.quant[k], pic.bytes[k], pic.quant[j], pic.bytes[j]), "%s: picture %d: quant[%d] overlaps "
              "quant[%d]", who, p, k, j);
      }
      ap.coeffs[k] = pic.coeffs[k];
      ap.quant[k] = have_quant ? pic.quant[k] : nullptr;
      ap.stride[k] = pic.stride[k];
      ap.width[k] = pic.iwt_width[k];
      ap.height[k] = pic.iwt_height[k];
      const int first = (int) plan.sbs.size ();
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
        s.pic = p;
        s.comp = k;
        s.index = i;
        plan.sbs.push_back (s);
      }
      // the component's towers: LL, and per orientation the levels from coarse to fine
      for (int o = 0; o < (depth ? 4 : 1); o++) {
        AdTower t = { first + o, o == 0 ? 1 : depth, p, 0 };
        int64_t samples = 0;
        for (int b = 0; b < t.nbands; b++)
          samples += (int64_t) plan.sbs[t.sb_first + 3 * b].bw * plan.sbs[t.sb_first + 3 * b].bh;
        plan.towers.push_back (t);
        work.push_back (samples);
      }
    }
    plan.pics.push_back (ap);
  }
  // the longest first (the finest orientations of the largest lumas), the LLs last: the long chains start at once, and where
  // a wave holds 64 towers (per_lane) they are of like length
  std::vector < int >order (plan.towers.size ());
  for (size_t n = 0; n < order.size (); n++)
    order[n] = (int) n;
  std::stable_sort (order.begin (), order.end (), [&work] (int a, int b) { return work[a] > work[b]; });
  std::vector < AdTower > sorted;
  for (int n:order)
    sorted.push_back (plan.towers[n]);
  plan.towers.swap (sorted);
  // what one picture writes (planes, result) may not touch what another reads or writes: the results are cleared in front of
  // the first launch, and all pictures run in every launch
  std::vector < AdRegion > regs;
  for (int p = 0; p < npictures; p++) {
    const SchroHipArithDecodePicture & pic = pictures[p];
    regs.push_back ({ (uintptr_t) pic.result, sizeof (SchroHipArithDecodeResult), p, true, "result" });
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
    std::sort (regs.begin (), regs.end (), [](const AdRegion & a, const AdRegion & b) { return a.at < b.at; });
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
schro_hip_arith_decode_check (const SchroHipArithDecodePicture * pictures, int npictures, int bytes_per_sample)
{
  AdPlan plan;
  return ad_build ("arith_decode_batch", pictures, npictures, bytes_per_sample, plan);
}

int64_t
schro_hip_arith_decode_scratch_words (const SchroHipArithDecodePicture * pictures, int npictures, int bytes_per_sample)
{
  AdPlan plan;
  const int r = ad_build ("arith_decode_scratch_words", pictures, npictures, bytes_per_sample, plan);
  if (r)
    return r;
  return (int64_t) kAdBandWords * (int64_t) plan.sbs.size ();
}

int
schro_hip_arith_decode_batch (SchroHipContext * ctx, const SchroHipArithDecodePicture * pictures, int npictures, int bytes_per_sample)
{
  const char *who = "arith_decode_batch";
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  AdPlan plan;
  int r = ad_build (who, pictures, npictures, bytes_per_sample, plan);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);

  // scratch of the selected queue: what the header launch finds, eight words per sub-band
  const size_t ns = plan.sbs.size (), npic = plan.pics.size (), nt = plan.towers.size ();
  r = ensure_scratch (ctx, kAdBandWords * ns * sizeof (uint32_t));
  if (r)
    return r;
  AdBand *bands = (AdBand *) ctx->scratch_ref ();

  // one table: the sub-bands, the pictures, the towers
  const size_t sb_bytes = ns * sizeof (NdSubband), pic_bytes = npic * sizeof (AdPicture), tw_bytes = nt * sizeof (AdTower);
  const size_t bytes = sb_bytes + pic_bytes + tw_bytes;
  static_assert (sizeof (NdSubband) % 8 == 0 && sizeof (AdPicture) % 8 == 0 && sizeof (AdBand) == 4 * kAdBandWords, "the table's parts");
  void *host, *dev;
  r = big_table_begin (ctx, bytes, &host, &dev);
  if (r)
    return r;
  memcpy (host, plan.sbs.data (), sb_bytes);
  memcpy ((char *) host + sb_bytes, plan.pics.data (), pic_bytes);
  memcpy ((char *) host + sb_bytes + pic_bytes, plan.towers.data (), tw_bytes);
  r = big_table_commit (ctx, bytes);
  if (r)
    return r;
  // (A/B runs, scripts/arith_decode_ab.py: one launch at a time on the tables the call before left; a tower per lane)
  const char *env = SCHRO_ENV ("SCHRO_HIP_ARDEC_STAGES");
  const int stages = env && atoi (env) > 0 ? atoi (env) & 7 : 7;
  env = SCHRO_ENV ("SCHRO_HIP_ARDEC_PER_LANE");
  const int per_lane = env && atoi (env) > 0;
  if (stages & 1)
    for (int p = 0; p < npictures; p++)
      SCHRO_HIP_CHECK (hipMemsetAsync (pictures[p].result, 0, sizeof (SchroHipArithDecodeResult), ctx->stream));
  return launch_arith_decode (ctx->stream, (const NdSubband *) dev, (const AdPicture *) ((const char *) dev + sb_bytes), npictures,
      (const AdTower *) ((const char *) dev + sb_bytes + pic_bytes), (int) nt, bands, bytes_per_sample, stages, per_lane);
}

}                               // extern "C"
