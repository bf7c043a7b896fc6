// plane_noarith_enc.cpp -- plane layer: core-syntax transform data in the VLC parse codes, written on the device
// (noarith_enc.hip).

#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

constexpr int64_t kNaMaxBound = (int64_t) 1 << 29;      // bit positions are 32-bit
constexpr int64_t kNaMaxUnits = (int64_t) 1 << 28;      // pieces and codeblocks of a call are indexed with int

struct NaBand {
  int position, shift, bw, bh, hc, vc;
};

// the refusals of a picture's sizes, depth and counts
int
na_check_geometry (const char *who, const SchroHipNoarithPicture & pic, int p)
{
  const int depth = pic.transform_depth;
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
  return 0;
}

NaBand
na_band (const SchroHipNoarithPicture & pic, int k, int index)
{
  NaBand b;
  b.position = index == 0 ? 0 : (((index - 1) / 3) << 2) | ((index - 1) % 3 + 1);
  const int level = b.position >> 2;    // SCHRO_SUBBAND_SHIFT
  b.shift = pic.transform_depth - level;
  b.bw = pic.iwt_width[k] >> b.shift;
  b.bh = pic.iwt_height[k] >> b.shift;
  b.hc = pic.horiz_codeblocks[index == 0 ? 0 : level + 1];
  b.vc = pic.vert_codeblocks[index == 0 ? 0 : level + 1];
  return b;
}

int64_t
na_bound (const SchroHipNoarithPicture & pic, int bpp)
{
  int64_t bound = 0;
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 1 + 3 * pic.transform_depth; i++) {
      const NaBand b = na_band (pic, k, i);
      // the codes; bit (zero) and sint (0) per codeblock and the flush; uint (length < 2^29), uint (quant index <= 60), a sync
      bound += (int64_t) b.bw * b.bh * 2 * bpp + ((int64_t) b.hc * b.vc * 2 + 7) / 8 + 10;
    }
  return bound;
}

struct NaPlan {
  std::vector < NaSubband > sbs;
  std::vector < NaPicture > pics;
  std::vector < int >sb_pic;
  int64_t pieces = 0, cbs = 0;
  int grid_x = 1, clear_x = 1;
};

int
na_build (const char *who, const SchroHipNoarithPicture * pictures, int npictures, int bpp, NaPlan & plan,
    const int32_t * const *chosen = nullptr, const uint32_t * clamped = nullptr, bool chosen_form = false)
{
  // the chosen form (schro_hip_noarith_encode_chosen_batch): a record's quant_index is its SUB-BAND, the index written
  // into the sub-band's header comes from chosen[picture][component][sub-band] on the device -- one per sub-band, so the
  // records of a sub-band cannot disagree; the sub-band records are completed by a resolve launch
  if (chosen_form) {
    SCHRO_HIP_REQUIRE (chosen && clamped && (uintptr_t) clamped % sizeof (uint32_t) == 0, "%s: chosen is NULL, or clamped is NULL or not "
        "4-byte aligned", who);
    for (int p = 0; pictures && p < npictures; p++)
      SCHRO_HIP_REQUIRE (chosen[p] && (uintptr_t) chosen[p] % sizeof (int32_t) == 0, "%s: picture %d: chosen is NULL or not 4-byte aligned",
          who, p);
  }
  SCHRO_HIP_REQUIRE (pictures && npictures > 0 && npictures <= kMaxJobs, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "%s: bytes_per_sample must be 2 or 4", who);
  for (int p = 0; p < npictures; p++) {
    const SchroHipNoarithPicture & pic = pictures[p];
    int r = na_check_geometry (who, pic, p);
    if (r)
      return r;
    const int depth = pic.transform_depth, nsub = 1 + 3 * depth;
    SCHRO_HIP_REQUIRE (pic.codeblock_mode_index == 0 || pic.codeblock_mode_index == 1, "%s: picture %d: codeblock_mode_index %d", who,
        p, pic.codeblock_mode_index);
    SCHRO_HIP_REQUIRE (pic.out, "%s: picture %d: out is NULL", who, p);
    SCHRO_HIP_REQUIRE (pic.result && (uintptr_t) pic.result % 4 == 0, "%s: picture %d: result is NULL or unaligned", who, p);
    const int64_t bound = na_bound (pic, bpp);
    SCHRO_HIP_REQUIRE (bound < kNaMaxBound, "%s: picture %d: a bound of %lld bytes, bit positions are 32-bit (below 2^29)", who, p,
        (long long) bound);
    NaPicture np;
    memset (&np, 0, sizeof (np));
    np.out = pic.out;
    np.result = pic.result;
    np.capacity = (uint32_t) std::min < uint64_t > (pic.capacity, (uint64_t) kNaMaxBound);
    np.sb_first = (int) plan.sbs.size ();
    np.nsb = 3 * nsub;
    np.cb_first = (int) plan.cbs;
    const uintptr_t o0 = (uintptr_t) pic.out, o1 = o0 + (size_t) std::min < uint64_t > (pic.capacity, (uint64_t) bound);
    int rows = 0;
    for (int k = 0; k < 3; k++) {
      SCHRO_HIP_REQUIRE (pic.quant[k] && (uintptr_t) pic.quant[k] % bpp == 0, "%s: picture %d: quant[%d] is NULL or misaligned", who, p, k);
      SCHRO_HIP_REQUIRE ((int64_t) pic.stride[k] >= (int64_t) pic.iwt_width[k] * bpp && pic.stride[k] % bpp == 0
          && ((int64_t) pic.stride[k] << depth) < ((int64_t) 1 << 31), "%s: picture %d: stride[%d] %d for %d samples of %d bytes", who, p,
          k, pic.stride[k], pic.iwt_width[k], bpp);
      SCHRO_HIP_REQUIRE (pic.codeblocks[k] && pic.ncodeblocks[k] > 0, "%s: picture %d: component %d has no records", who, p, k);
      const uintptr_t q0 = (uintptr_t) pic.quant[k], q1 = q0 + pic.bytes[k];
      SCHRO_HIP_REQUIRE (o1 <= q0 || q1 <= o0, "%s: picture %d: out overlaps quant[%d]", who, p, k);
      int64_t expect = 0;
      for (int i = 0; i < nsub; i++) {
        const NaBand b = na_band (pic, k, i);
        expect += (int64_t) b.hc * b.vc;
      }
      SCHRO_HIP_REQUIRE (expect == pic.ncodeblocks[k], "%s: picture %d, component %d: %d records, the stated counts make %lld", who, p, k,
          pic.ncodeblocks[k], (long long) expect);
      int n = 0;
      for (int i = 0; i < nsub; i++) {
        const NaBand b = na_band (pic, k, i);
        const int bstride = pic.stride[k] << b.shift;
        const int base = ((b.position & 2) ? bstride >> 1 : 0) + ((b.position & 1) ? b.bw * bpp : 0);
        SCHRO_HIP_REQUIRE ((int64_t) base + (int64_t) (b.bh - 1) * bstride + (int64_t) b.bw * bpp <= (int64_t) pic.bytes[k],
            "%s: picture %d, component %d, sub-band %d (%d x %d at byte %d, pitch %d) reaches outside the plane's %zu bytes", who, p, k,
            i, b.bw, b.bh, base, bstride, pic.bytes[k]);
        const int qi = pic.codeblocks[k][n].quant_index;
        for (int y = 0; y < b.vc; y++) {
          const int ymin = (b.bh * y) / b.vc, ymax = (b.bh * (y + 1)) / b.vc;
          for (int x = 0; x < b.hc; x++, n++) {
            const SchroHipCodeblock & cb = pic.codeblocks[k][n];
            const int xmin = (b.bw * x) / b.hc, xmax = (b.bw * (x + 1)) / b.hc;
            SCHRO_HIP_REQUIRE (cb.dst_offset == base + ymin * bstride + xmin * bpp && cb.dst_stride == bstride && cb.width == xmax - xmin
                && cb.height == ymax - ymin,
                "%s: picture %d, component %d, sub-band %d, record %d (%d x %d at byte %d, pitch %d) is not schro_hip_codeblock_layout's "
                "(%d x %d at byte %d, pitch %d)", who, p, k, i, n, cb.width, cb.height, cb.dst_offset, cb.dst_stride, xmax - xmin,
                ymax - ymin, base + ymin * bstride + xmin * bpp, bstride);
            if (chosen_form) {
              SCHRO_HIP_REQUIRE (cb.quant_index == i, "%s: picture %d, component %d, sub-band %d, record %d: quant_index %d is not the "
                  "sub-band", who, p, k, i, n, cb.quant_index);
              continue;
            }
            SCHRO_HIP_REQUIRE (cb.quant_index <= 60, "%s: picture %d, component %d, sub-band %d, record %d: quant_index %d", who, p, k, i,
                n, cb.quant_index);
            // the quant offset written is always 0 (schroencoder.c:4148-4150): unlike indices would decode wrongly
            SCHRO_HIP_REQUIRE (cb.quant_index == qi, "%s: picture %d, component %d, sub-band %d: record %d has quant index %d, codeblock "
                "(0, 0) has %d: the quant offset written is always 0", who, p, k, i, n, cb.quant_index, qi);
          }
        }
        NaSubband s;
        memset (&s, 0, sizeof (s));
        s.base = (const char *) pic.quant[k] + base;
        s.stride = bstride;
        s.bw = b.bw;
        s.bh = b.bh;
        s.hc = b.hc;
        s.vc = b.vc;
        s.piece_base = (int) plan.pieces;
        s.cb_base = (int) plan.cbs;
        s.row_base = rows;
        const bool many = b.hc > 1 || b.vc > 1;
        s.flags = (many && i > 0 ? 1 : 0) | (many && pic.codeblock_mode_index == 1 ? 2 : 0);
        s.quant_index = chosen_form ? 0 : qi;
        s.comp = k;
        s.index = i;
        plan.sbs.push_back (s);
        plan.sb_pic.push_back (p);
        plan.pieces += (int64_t) b.bh * b.hc;
        plan.cbs += (int64_t) b.hc * b.vc;
        rows += b.bh;
        plan.grid_x = (int) std::min < int64_t > (kNaGridX, std::max < int64_t > (plan.grid_x, (int64_t) b.bh * b.hc + (b.hc * b.vc + 63) / 64));
        SCHRO_HIP_REQUIRE (plan.pieces < kNaMaxUnits && plan.cbs < kNaMaxUnits, "%s: picture %d: more than 2^28 row pieces or codeblocks "
            "in one call", who, p);
      }
    }
    np.ncb = (int) plan.cbs - np.cb_first;
    np.rows = rows;
    plan.pics.push_back (np);
    // the clear launch: 4 KiB of output per workgroup, over the most a picture can take
    const int64_t most = std::min < int64_t > (bound, (int64_t) np.capacity) + 3;
    plan.clear_x = (int) std::max < int64_t > (plan.clear_x, (most + 4095) / 4096);
  }
  return 0;
}

}                               // namespace

extern "C" {

int64_t
schro_hip_noarith_encode_bound (const SchroHipNoarithPicture * picture, int bytes_per_sample)
{
  SCHRO_HIP_REQUIRE (picture, "noarith_encode_bound: bad arguments");
  SCHRO_HIP_REQUIRE (bytes_per_sample == 2 || bytes_per_sample == 4, "noarith_encode_bound: bytes_per_sample must be 2 or 4");
  int r = na_check_geometry ("noarith_encode_bound", *picture, 0);
  if (r)
    return r;
  return na_bound (*picture, bytes_per_sample);
}

int
schro_hip_noarith_encode_check (const SchroHipNoarithPicture * pictures, int npictures, int bytes_per_sample)
{
  NaPlan plan;
  return na_build ("noarith_encode_batch", pictures, npictures, bytes_per_sample, plan);
}

}                               // extern "C"

static int
na_encode_run (const char *who, SchroHipContext * ctx, const SchroHipNoarithPicture * pictures, int npictures, int bytes_per_sample,
    const int32_t * const *chosen, uint32_t * clamped, bool chosen_form)
{
  SCHRO_HIP_REQUIRE (ctx, "%s: bad arguments", who);
  NaPlan plan;
  int r = na_build (who, pictures, npictures, bytes_per_sample, plan, chosen, clamped, chosen_form);
  if (r)
    return r;
  (void) hipSetDevice (ctx->device);

  // scratch of the selected queue: three words per piece, four per codeblock, two per sub-band
  const size_t np = (size_t) plan.pieces, nc = (size_t) plan.cbs, ns = plan.sbs.size ();
  r = ensure_scratch (ctx, (3 * np + 4 * nc + 2 * ns) * sizeof (uint32_t));
  if (r)
    return r;
  uint32_t *w = (uint32_t *) ctx->scratch_ref ();
  NaScratch S;
  S.bits = w;
  S.info = w + np;
  S.start = w + 2 * np;
  w += 3 * np;
  S.cb_bits = w;
  S.cb_flags = w + nc;
  S.cb_pos = w + 2 * nc;
  S.cb_at = w + 3 * nc;
  w += 4 * nc;
  S.sb_at = w;
  S.sb_len = w + ns;

  // one table: the sub-bands, the pictures, the picture of every sub-band
  const size_t sb_bytes = ns * sizeof (NaSubband), pic_bytes = plan.pics.size () * sizeof (NaPicture);
  const size_t index_bytes = round_up (ns * sizeof (int), sizeof (void *));
  const size_t bytes = sb_bytes + pic_bytes + index_bytes + (chosen_form ? (size_t) npictures * sizeof (void *) : 0);
  void *host, *dev;
  r = big_table_begin (ctx, bytes, &host, &dev);
  if (r)
    return r;
  memcpy (host, plan.sbs.data (), sb_bytes);
  memcpy ((char *) host + sb_bytes, plan.pics.data (), pic_bytes);
  memcpy ((char *) host + sb_bytes + pic_bytes, plan.sb_pic.data (), ns * sizeof (int));
  if (chosen_form)
    memcpy ((char *) host + sb_bytes + pic_bytes + index_bytes, chosen, (size_t) npictures * sizeof (void *));
  r = big_table_commit (ctx, bytes);
  if (r)
    return r;
  if (chosen_form) {
    r = launch_noarith_resolve (ctx->stream, (NaSubband *) dev, (int) ns, (const int *) ((const char *) dev + sb_bytes + pic_bytes),
        (const int32_t * const *) ((const char *) dev + sb_bytes + pic_bytes + index_bytes), clamped);
    if (r)
      return r;
  }
  // (A/B runs, scripts/noarith_encode_ab.py: one launch at a time on the tables the call before left)
  const char *env = SCHRO_ENV ("SCHRO_HIP_NAENC_STAGES");
  const int stages = env && atoi (env) > 0 ? atoi (env) & 7 : 7;
  if (stages & 2)
    for (int p = 0; p < npictures; p++)
      SCHRO_HIP_CHECK (hipMemsetAsync (pictures[p].result, 0, sizeof (SchroHipNoarithResult), ctx->stream));
  return launch_noarith_encode (ctx->stream, (const NaSubband *) dev, (int) ns, (const NaPicture *) ((const char *) dev + sb_bytes),
      npictures, S, bytes_per_sample, plan.grid_x, plan.clear_x, stages);
}

extern "C" {

int
schro_hip_noarith_encode_batch (SchroHipContext * ctx, const SchroHipNoarithPicture * pictures, int npictures, int bytes_per_sample)
{
  return na_encode_run ("noarith_encode_batch", ctx, pictures, npictures, bytes_per_sample, nullptr, nullptr, false);
}

int
schro_hip_noarith_encode_chosen_batch (SchroHipContext * ctx, const SchroHipNoarithPicture * pictures, const int32_t * const *chosen,
    int npictures, int bytes_per_sample, uint32_t * clamped)
{
  return na_encode_run ("noarith_encode_chosen_batch", ctx, pictures, npictures, bytes_per_sample, chosen, clamped, true);
}

int
schro_hip_noarith_encode_chosen_check (const SchroHipNoarithPicture * pictures, const int32_t * const *chosen, int npictures,
    int bytes_per_sample, const uint32_t * clamped)
{
  NaPlan plan;
  return na_build ("noarith_encode_chosen_batch", pictures, npictures, bytes_per_sample, plan, chosen, clamped, true);
}

}                               // extern "C"
