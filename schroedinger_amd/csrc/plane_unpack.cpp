// plane_unpack.cpp -- plane layer: the encoder's way in.  schro_hip_unpack_batch, the encoder-direction
// schro_frame_convert (unpack.hip), and schro_hip_unpack_iwt_batch, an intra picture from packed bytes to wavelet
// coefficients (the level-0 launch of iwt_fwd.hip with the packed fetch stage, or the chain through the queue's block).
//
// Routes of schro_hip_unpack_iwt_batch, per picture (schro_hip_unpack_routes):
//   FUSED     the format x sample type x filter combinations of kFusedFilters below (the measured ones), when the
//             transform's chroma format is the packed format's own and the packed pointer and stride are multiples of 16
//   TWO_PASS  everything else (the other combinations, a chroma change, other alignments)

#include "schro_hip_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace {

bool
env_on (const char *v)
{
  return v && *v && strcmp (v, "0") != 0;
}

struct PackedForm {
  int depth;                    // bytes per sample of the unpacked frame
  int hs, vs;                   // its chroma shifts
  const char *name;
};

// schro_virt_frame_new_unpack's table (schrovirtframe.c:902-933)
bool
packed_form (int format, PackedForm * f)
{
  switch (format) {
    case SCHRO_HIP_FORMAT_YUYV: *f = { 1, 1, 0, "YUYV" }; return true;
    case SCHRO_HIP_FORMAT_UYVY: *f = { 1, 1, 0, "UYVY" }; return true;
    case SCHRO_HIP_FORMAT_AYUV: *f = { 1, 0, 0, "AYUV" }; return true;
    case SCHRO_HIP_FORMAT_v210: *f = { 2, 1, 0, "v210" }; return true;
    case SCHRO_HIP_FORMAT_v216: *f = { 2, 1, 0, "v216" }; return true;
    case SCHRO_HIP_FORMAT_AY64: *f = { 4, 0, 0, "AY64" }; return true;
  }
  return false;
}

// the bytes of a packed row the unpack reads
int
packed_row_bytes (int format, int width)
{
  switch (format) {
    case SCHRO_HIP_FORMAT_YUYV:
    case SCHRO_HIP_FORMAT_UYVY: return 4 * (width / 2);
    case SCHRO_HIP_FORMAT_AYUV: return 4 * width;
    case SCHRO_HIP_FORMAT_v210: return 16 * div_up (width, 6);
    case SCHRO_HIP_FORMAT_v216: return 8 * (width / 2);
    default: return 8 * width;  // AY64
  }
}

int
shifted (int v, int shift)
{
  return (v + (1 << shift) - 1) >> shift;
}

bool
shifts_ok (int hs, int vs)
{
  return (hs | vs) >= 0 && hs <= 1 && vs <= 1 && !(vs && !hs);
}

// where component k of a packed picture lies in its rows (unpack_fetch.h)
void
packed_src (UnpackSrc & s, int format, int k, const void *base, int stride, int src_width)
{
  PackedForm f;
  packed_form (format, &f);
  memset (&s, 0, sizeof (s));
  s.base = (const uint8_t *) base;
  s.stride = stride;
  s.row_bytes = packed_row_bytes (format, src_width);
  s.depth = f.depth;
  s.comp = k;
  s.kind = kUnpackU8;
  switch (format) {
    case SCHRO_HIP_FORMAT_YUYV:        // Y0 U Y1 V
      s.xmul = k ? 4 : 2;
      s.xoff = k == 0 ? 0 : k == 1 ? 1 : 3;
      break;
    case SCHRO_HIP_FORMAT_UYVY:        // U Y0 V Y1
      s.xmul = k ? 4 : 2;
      s.xoff = k == 0 ? 1 : k == 1 ? 0 : 2;
      break;
    case SCHRO_HIP_FORMAT_AYUV:
      s.xmul = 4;
      s.xoff = 1 + k;
      break;
    case SCHRO_HIP_FORMAT_v210:
      s.kind = kUnpackV210;
      break;
    case SCHRO_HIP_FORMAT_v216:        // U Y0 V Y1, 16-bit words: the high byte
      s.xmul = k ? 8 : 4;
      s.xoff = k == 0 ? 3 : k == 1 ? 1 : 5;
      break;
    default:                           // AY64: A Y U V, 16-bit words
      s.kind = kUnpackU16;
      s.xmul = 8;
      s.xoff = 2 + 2 * k;
      break;
  }
}

// Which packed format x sample type x filter takes FUSED in the product library: where scripts/unpack_iwt_ab.py --sweep
// (8 x 2160p, depth 3; profiles/unpack_iwt.txt) did NOT measure the packed level 0 slower than the chain by more than the
// larger of the two forms' spreads.  Bit f of the entry: filter f.  tests/test_gpu_unpack_iwt.py holds the same table.
//                                   s16   s32
const uint8_t kFusedFilters[6][2] = {
  { 0x18, 0x5f },               // YUYV: Haar0, Haar1; all but Fidelity
  { 0x18, 0x5f },               // UYVY
  { 0x18, 0x5f },               // AYUV
  { 0x18, 0x5f },               // v210
  { 0x18, 0x5f },               // v216
  { 0x5f, 0x7f },               // AY64: all but Fidelity; all
};

bool
unpack_fused_combination (int format, int bpp, int filter)
{
  const int col = bpp == 2 ? 0 : 1;
  switch (format) {
    case SCHRO_HIP_FORMAT_YUYV: return (kFusedFilters[0][col] >> filter) & 1;
    case SCHRO_HIP_FORMAT_UYVY: return (kFusedFilters[1][col] >> filter) & 1;
    case SCHRO_HIP_FORMAT_AYUV: return (kFusedFilters[2][col] >> filter) & 1;
    case SCHRO_HIP_FORMAT_v210: return (kFusedFilters[3][col] >> filter) & 1;
    case SCHRO_HIP_FORMAT_v216: return (kFusedFilters[4][col] >> filter) & 1;
    case SCHRO_HIP_FORMAT_AY64: return (kFusedFilters[5][col] >> filter) & 1;
  }
  return false;
}

struct Span {
  uintptr_t begin, end;
};

Span
span_of (const void *p, int stride, int row_bytes, int rows)
{
  const uintptr_t b = (uintptr_t) p;
  return { b, b + (uintptr_t) stride * (uintptr_t) (rows - 1) + (uintptr_t) row_bytes };
}

}                               // namespace

extern "C" {

int
schro_hip_unpack_batch (SchroHipContext * ctx, const SchroHipUnpackPicture * pictures, int npictures)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && npictures > 0, "unpack_batch: bad arguments");
  SCHRO_HIP_REQUIRE (npictures <= SCHRO_HIP_UNPACK_MAX_PICTURES, "unpack_batch: at most %d pictures per call",
      SCHRO_HIP_UNPACK_MAX_PICTURES);
  (void) hipSetDevice (ctx->device);
  int px, rows;
  unpack_tile_geometry (&px, &rows);
  std::vector < UnpackJob > jobs ((size_t) 3 * npictures);
  std::vector < Span > reads, writes;
  int tile_base = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipUnpackPicture & pc = pictures[p];
    SCHRO_HIP_REQUIRE (pc.width > 0 && pc.height > 0 && pc.src_width > 0 && pc.src_height > 0,
        "unpack_batch: picture %d: sizes %dx%d from %dx%d must be positive", p, pc.width, pc.height, pc.src_width, pc.src_height);
    SCHRO_HIP_REQUIRE (pc.width <= (1 << 17) && pc.height <= (1 << 17) && pc.src_width <= (1 << 17) && pc.src_height <= (1 << 17),
        "unpack_batch: picture %d is too large", p);
    SCHRO_HIP_REQUIRE (pc.format != SCHRO_HIP_FORMAT_ARGB,
        "unpack_batch: picture %d: ARGB sources are refused: unpack_argb writes 16-bit samples into the lines of a frame "
        "labelled U8_444 (schrovirtframe.c:693-732, 927-929)", p);
    PackedForm f = { pc.src_bpp, pc.src_h_shift, pc.src_v_shift, "planar" };
    const bool packed = pc.format != 0;
    SCHRO_HIP_REQUIRE (!packed || packed_form (pc.format, &f), "unpack_batch: picture %d: format 0x%x is no packed format", p,
        pc.format);
    SCHRO_HIP_REQUIRE (f.depth == 1 || f.depth == 2 || f.depth == 4, "unpack_batch: picture %d: src_bpp must be 1, 2 or 4", p);
    SCHRO_HIP_REQUIRE (pc.dst_bpp == 1 || pc.dst_bpp == 2 || pc.dst_bpp == 4, "unpack_batch: picture %d: dst_bpp must be 1, 2 or 4", p);
    SCHRO_HIP_REQUIRE (shifts_ok (f.hs, f.vs) && shifts_ok (pc.h_shift, pc.v_shift),
        "unpack_batch: picture %d: chroma format not 4:4:4 / 4:2:2 / 4:2:0", p);
    SCHRO_HIP_REQUIRE (!(pc.format == SCHRO_HIP_FORMAT_AY64 && pc.dst_bpp == 1),
        "unpack_batch: picture %d: AY64 -> u8 is refused: schroframe.c:908 tests the depth of the packed format code "
        "(0x107 & 0xc: S16) and reads the s32 lines as s16", p);
    SCHRO_HIP_REQUIRE (!((pc.format == SCHRO_HIP_FORMAT_YUYV || pc.format == SCHRO_HIP_FORMAT_UYVY
                || pc.format == SCHRO_HIP_FORMAT_v216) && (pc.src_width & 1)),
        "unpack_batch: picture %d: %s of odd width %d is refused: the reference unpacks width / 2 chroma samples of a "
        "(width + 1) / 2 wide component (schrovirtframe.c:629, 652, 881)", p, f.name, pc.src_width);
    const bool chroma_change = f.hs != pc.h_shift || f.vs != pc.v_shift;
    SCHRO_HIP_REQUIRE (!(chroma_change && pc.dst_bpp != 1),
        "unpack_batch: picture %d: a chroma change on an s16 / s32 frame is refused: schro_virt_frame_new_subsample "
        "resamples u8 frames only (schrovirtframe.c:1549-1569)", p);
    SCHRO_HIP_REQUIRE (!((pc.width < pc.src_width || pc.height < pc.src_height)
            && (pc.width > pc.src_width || pc.height > pc.src_height)),
        "unpack_batch: picture %d: %dx%d from %dx%d mixes crop and extension (schrovirtframe.c:1861-1862, 1939-1940)", p,
        pc.width, pc.height, pc.src_width, pc.src_height);
    for (int k = 0; k < 3; k++) {
      const int hs_d = k ? pc.h_shift : 0, vs_d = k ? pc.v_shift : 0;
      const int hs_s = k ? f.hs : 0, vs_s = k ? f.vs : 0;
      UnpackJob & j = jobs[(size_t) 3 * p + k];
      memset (&j, 0, sizeof (j));
      SCHRO_HIP_REQUIRE (pc.dst[k], "unpack_batch: picture %d: dst[%d] is NULL", p, k);
      if (packed) {
        SCHRO_HIP_REQUIRE (pc.src[0], "unpack_batch: picture %d: src[0] is NULL", p);
        packed_src (j.s, pc.format, k, pc.src[0], pc.src_stride[0], pc.src_width);
        SCHRO_HIP_REQUIRE (pc.src_stride[0] >= j.s.row_bytes, "unpack_batch: picture %d: source stride %d below a row of %d bytes",
            p, pc.src_stride[0], j.s.row_bytes);
        SCHRO_HIP_REQUIRE (pc.format != SCHRO_HIP_FORMAT_AY64 || (((uintptr_t) pc.src[0] | (uintptr_t) pc.src_stride[0]) & 1) == 0,
            "unpack_batch: picture %d: AY64 rows must be 2-byte aligned", p);
        if (k == 0)
          reads.push_back (span_of (pc.src[0], pc.src_stride[0], j.s.row_bytes, pc.src_height));
      } else {
        const int cw = shifted (pc.src_width, hs_s), chh = shifted (pc.src_height, vs_s);
        SCHRO_HIP_REQUIRE (pc.src[k], "unpack_batch: picture %d: src[%d] is NULL", p, k);
        SCHRO_HIP_REQUIRE (pc.src_stride[k] >= cw * f.depth, "unpack_batch: picture %d: source stride %d of component %d below a row",
            p, pc.src_stride[k], k);
        SCHRO_HIP_REQUIRE ((((uintptr_t) pc.src[k] | (uintptr_t) pc.src_stride[k]) & (uintptr_t) (f.depth - 1)) == 0,
            "unpack_batch: picture %d: source component %d is not aligned to its %d-byte samples", p, k, f.depth);
        j.s.base = (const uint8_t *) pc.src[k];
        j.s.stride = pc.src_stride[k];
        j.s.row_bytes = cw * f.depth;
        j.s.kind = f.depth == 1 ? kUnpackU8 : f.depth == 2 ? kUnpackS16 : kUnpackS32;
        j.s.xmul = f.depth;
        j.s.depth = f.depth;
        reads.push_back (span_of (pc.src[k], pc.src_stride[k], j.s.row_bytes, chh));
      }
      j.dst = (uint8_t *) pc.dst[k];
      j.dst_stride = pc.dst_stride[k];
      j.dst_bpp = pc.dst_bpp;
      j.w = shifted (pc.width, hs_d);
      j.h = shifted (pc.height, vs_d);
      SCHRO_HIP_REQUIRE (pc.dst_stride[k] >= j.w * pc.dst_bpp, "unpack_batch: picture %d: destination stride %d of component %d below a row",
          p, pc.dst_stride[k], k);
      SCHRO_HIP_REQUIRE ((((uintptr_t) pc.dst[k] | (uintptr_t) pc.dst_stride[k]) & (uintptr_t) (pc.dst_bpp - 1)) == 0,
          "unpack_batch: picture %d: destination component %d is not aligned to its %d-byte samples", p, k, pc.dst_bpp);
      // the frame the crop / extension reads: the source's size in the destination's chroma format
      j.xmax = shifted (pc.src_width, hs_d) - 1;
      j.ymax = shifted (pc.src_height, vs_d) - 1;
      j.xsh = hs_d - hs_s;
      j.ysh = vs_d - vs_s;
      j.vec = (((uintptr_t) pc.dst[k] | (uintptr_t) pc.dst_stride[k]) & 15) == 0;
      j.tiles_x = div_up (div_up (j.w * pc.dst_bpp, 16), px);
      j.tile_base = tile_base;
      tile_base += j.tiles_x * div_up (j.h, rows);
      writes.push_back (span_of (pc.dst[k], pc.dst_stride[k], j.w * pc.dst_bpp, j.h));
    }
  }
  for (size_t a = 0; a < writes.size (); a++)
    for (size_t b = 0; b < reads.size (); b++)
      SCHRO_HIP_REQUIRE (writes[a].end <= reads[b].begin || reads[b].end <= writes[a].begin,
          "unpack_batch: picture %d: destination component %d overlaps a source of the call", (int) a / 3, (int) a % 3);
  void *d_jobs;
  int r = push_args (ctx, jobs.data (), sizeof (UnpackJob) * jobs.size (), &d_jobs);
  if (r)
    return r;
  ProfileScope ps (ctx, SCHRO_HIP_KERNEL_CONVERT);
  return launch_unpack (ctx->stream, (const UnpackJob *) d_jobs, (int) jobs.size (), tile_base);
}

int
schro_hip_unpack_iwt_batch (SchroHipContext * ctx, const SchroHipUnpackIwtPicture * pictures, int npictures, int depth, int filter,
    int bpp)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && npictures > 0, "unpack_iwt_batch: bad arguments");
  SCHRO_HIP_REQUIRE (npictures <= SCHRO_HIP_UNPACK_MAX_PICTURES, "unpack_iwt_batch: at most %d pictures per call",
      SCHRO_HIP_UNPACK_MAX_PICTURES);
  SCHRO_HIP_REQUIRE (depth >= 1 && depth <= 6, "unpack_iwt_batch: transform depth %d out of range", depth);
  SCHRO_HIP_REQUIRE (filter >= 0 && filter <= 6, "unpack_iwt_batch: wavelet filter index %d out of range", filter);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "unpack_iwt_batch: bytes_per_sample must be 2 or 4");
  (void) hipSetDevice (ctx->device);
  // (experiments: SCHRO_HIP_UNPACK_TWO_PASS=1 sends every picture to the two passes, SCHRO_HIP_UNPACK_FUSED=1 every
  // combination that allows it to the packed level 0, for A/B runs and the tests of both routes)
  const bool fused_on = !env_on (SCHRO_ENV ("SCHRO_HIP_UNPACK_TWO_PASS")), fused_all = env_on (SCHRO_ENV ("SCHRO_HIP_UNPACK_FUSED"));

  // ---- every refusal of the chain, the routes and the chain's frames, before anything is launched or counted ---------
  // a TWO_PASS picture has frame A (the picture in the packed format's own depth) and frame B (the transform size, bpp)
  // in the queue's block
  struct Slot {
    size_t off;
    int stride;
  };
  std::vector < Slot > slot_a ((size_t) 3 * npictures), slot_b ((size_t) 3 * npictures);
  std::vector < PackedForm > form (npictures);
  std::vector < int >fused (npictures, 0);
  size_t total = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipUnpackIwtPicture & pc = pictures[p];
    PackedForm & f = form[p];
    SCHRO_HIP_REQUIRE (pc.format != SCHRO_HIP_FORMAT_ARGB,
        "unpack_iwt_batch: picture %d: ARGB sources are refused: unpack_argb writes 16-bit samples into the lines of a "
        "frame labelled U8_444 (schrovirtframe.c:693-732, 927-929)", p);
    SCHRO_HIP_REQUIRE (packed_form (pc.format, &f), "unpack_iwt_batch: picture %d: format 0x%x is no packed format", p, pc.format);
    SCHRO_HIP_REQUIRE (pc.src && pc.width > 0 && pc.height > 0 && pc.src_width > 0 && pc.src_height > 0 && pc.iwt_width > 0
        && pc.iwt_height > 0, "unpack_iwt_batch: picture %d: a NULL source or a size that is not positive", p);
    SCHRO_HIP_REQUIRE (pc.src_width <= (1 << 17) && pc.src_height <= (1 << 17) && pc.iwt_width <= (1 << 17) && pc.iwt_height <= (1 << 17),
        "unpack_iwt_batch: picture %d is too large", p);
    SCHRO_HIP_REQUIRE (shifts_ok (pc.h_shift, pc.v_shift), "unpack_iwt_batch: picture %d: chroma format not 4:4:4 / 4:2:2 / 4:2:0", p);
    SCHRO_HIP_REQUIRE (!((pc.format == SCHRO_HIP_FORMAT_YUYV || pc.format == SCHRO_HIP_FORMAT_UYVY
                || pc.format == SCHRO_HIP_FORMAT_v216) && (pc.src_width & 1)),
        "unpack_iwt_batch: picture %d: %s of odd width %d is refused: the reference unpacks width / 2 chroma samples of a "
        "(width + 1) / 2 wide component (schrovirtframe.c:629, 652, 881)", p, f.name, pc.src_width);
    const bool chroma_change = f.hs != pc.h_shift || f.vs != pc.v_shift;
    SCHRO_HIP_REQUIRE (!(chroma_change && f.depth != 1),
        "unpack_iwt_batch: picture %d: a chroma change on an s16 / s32 frame is refused: schro_virt_frame_new_subsample "
        "resamples u8 frames only (schrovirtframe.c:1549-1569)", p);
    SCHRO_HIP_REQUIRE (!((pc.width < pc.src_width || pc.height < pc.src_height)
            && (pc.width > pc.src_width || pc.height > pc.src_height)),
        "unpack_iwt_batch: picture %d: %dx%d from %dx%d mixes crop and extension (schrovirtframe.c:1861-1862, 1939-1940)", p,
        pc.width, pc.height, pc.src_width, pc.src_height);
    SCHRO_HIP_REQUIRE (pc.iwt_width >= pc.width && pc.iwt_height >= pc.height,
        "unpack_iwt_batch: picture %d: the transform size %dx%d does not hold the picture %dx%d", p, pc.iwt_width, pc.iwt_height,
        pc.width, pc.height);
    const int row_bytes = packed_row_bytes (pc.format, pc.src_width);
    SCHRO_HIP_REQUIRE (pc.src_stride >= row_bytes, "unpack_iwt_batch: picture %d: source stride %d below a row of %d bytes", p,
        pc.src_stride, row_bytes);
    SCHRO_HIP_REQUIRE (pc.format != SCHRO_HIP_FORMAT_AY64 || (((uintptr_t) pc.src | (uintptr_t) pc.src_stride) & 1) == 0,
        "unpack_iwt_batch: picture %d: AY64 rows must be 2-byte aligned", p);
    const Span s = span_of (pc.src, pc.src_stride, row_bytes, pc.src_height);
    fused[p] = fused_on && (fused_all || unpack_fused_combination (pc.format, bpp, filter)) && !chroma_change
        && (((uintptr_t) pc.src | (uintptr_t) pc.src_stride) & 15) == 0;
    for (int k = 0; k < 3; k++) {
      const int hs = k ? pc.h_shift : 0, vs = k ? pc.v_shift : 0;
      const int w = shifted (pc.iwt_width, hs), h = shifted (pc.iwt_height, vs);
      // (what schro_hip_iwt_batch refuses)
      SCHRO_HIP_REQUIRE (pc.dst[k], "unpack_iwt_batch: picture %d: dst[%d] is NULL", p, k);
      SCHRO_HIP_REQUIRE (w % (1 << depth) == 0 && h % (1 << depth) == 0,
          "unpack_iwt_batch: picture %d: component %d size %dx%d is not a multiple of 2^depth", p, k, w, h);
      SCHRO_HIP_REQUIRE (pc.dst_stride[k] >= w * bpp, "unpack_iwt_batch: picture %d: component %d stride too small", p, k);
      SCHRO_HIP_REQUIRE (pc.dst_stride[k] % bpp == 0 && (uintptr_t) pc.dst[k] % bpp == 0,
          "unpack_iwt_batch: picture %d: component %d: pointer and stride must be multiples of the sample size %d", p, k, bpp);
      const Span d = span_of (pc.dst[k], pc.dst_stride[k], w * bpp, h);
      SCHRO_HIP_REQUIRE (d.end <= s.begin || s.end <= d.begin, "unpack_iwt_batch: picture %d: component %d overlaps the source", p, k);
      Slot & sa = slot_a[(size_t) 3 * p + k], &sb = slot_b[(size_t) 3 * p + k];
      sa.stride = (int) round_up ((size_t) shifted (pc.width, hs) * f.depth, 128);
      sb.stride = (int) round_up ((size_t) w * bpp, 128);
      if (!fused[p]) {
        sa.off = total;
        total += round_up ((size_t) sa.stride * shifted (pc.height, vs), 256);
        sb.off = total;
        total += round_up ((size_t) sb.stride * h, 256);
      }
    }
  }

  char *block = nullptr;
  if (total) {
    const int q = ctx->cur;
    int r = grow_block (ctx, ctx->pack_tmp_q[q], ctx->pack_tmp_size_q[q], total);
    if (r)
      return r;
    block = (char *) ctx->pack_tmp_q[q];
  }

  // ---- TWO_PASS: the two converts of every such picture, one launch each ----------------------------------------
  std::vector < SchroHipUnpackPicture > ca, cb;
  for (int p = 0; p < npictures; p++) {
    if (fused[p])
      continue;
    const SchroHipUnpackIwtPicture & pc = pictures[p];
    SchroHipUnpackPicture a, b;
    memset (&a, 0, sizeof (a));
    memset (&b, 0, sizeof (b));
    a.src[0] = pc.src;
    a.src_stride[0] = pc.src_stride;
    a.format = pc.format;
    a.src_width = pc.src_width;
    a.src_height = pc.src_height;
    a.dst_bpp = b.src_bpp = form[p].depth;
    a.h_shift = b.src_h_shift = b.h_shift = pc.h_shift;
    a.v_shift = b.src_v_shift = b.v_shift = pc.v_shift;
    a.width = b.src_width = pc.width;
    a.height = b.src_height = pc.height;
    b.dst_bpp = bpp;
    b.width = pc.iwt_width;
    b.height = pc.iwt_height;
    for (int k = 0; k < 3; k++) {
      const Slot & sa = slot_a[(size_t) 3 * p + k], &sb = slot_b[(size_t) 3 * p + k];
      a.dst[k] = block + sa.off;
      a.dst_stride[k] = sa.stride;
      b.src[k] = block + sa.off;
      b.src_stride[k] = sa.stride;
      b.dst[k] = block + sb.off;
      b.dst_stride[k] = sb.stride;
    }
    ca.push_back (a);
    cb.push_back (b);
  }
  if (!ca.empty ()) {
    int r = schro_hip_unpack_batch (ctx, ca.data (), (int) ca.size ());
    if (!r)
      r = schro_hip_unpack_batch (ctx, cb.data (), (int) cb.size ());
    if (r)
      return r;
  }

  // ---- the transform: level 0 of the FUSED pictures reads the packed rows, the rest is the level loop's ----------------
  std::vector < SchroHipIwtFwdPlane > planes ((size_t) 3 * npictures);
  std::vector < IwtFwdPacked > packed ((size_t) 3 * npictures);
  for (int p = 0; p < npictures; p++) {
    const SchroHipUnpackIwtPicture & pc = pictures[p];
    for (int k = 0; k < 3; k++) {
      const int hs = k ? pc.h_shift : 0, vs = k ? pc.v_shift : 0;
      SchroHipIwtFwdPlane & pl = planes[(size_t) 3 * p + k];
      IwtFwdPacked & pk = packed[(size_t) 3 * p + k];
      memset (&pl, 0, sizeof (pl));
      memset (&pk, 0, sizeof (pk));
      pl.dst = pc.dst[k];
      pl.dst_stride = pc.dst_stride[k];
      pl.width = shifted (pc.iwt_width, hs);
      pl.height = shifted (pc.iwt_height, vs);
      if (fused[p]) {
        pk.packed = true;
        packed_src (pk.s, pc.format, k, pc.src, pc.src_stride, pc.src_width);
        // the two clamps of the chain, picture then source, are one
        pk.xmax = std::min (shifted (pc.width, hs), shifted (pc.src_width, hs)) - 1;
        pk.ymax = std::min (shifted (pc.height, vs), shifted (pc.src_height, vs)) - 1;
      } else {
        const Slot & sb = slot_b[(size_t) 3 * p + k];
        pl.src = block + sb.off;
        pl.src_stride = sb.stride;
      }
    }
  }
  int r = iwt_batch_run (ctx, planes.data (), (int) planes.size (), depth, filter, bpp, false, packed.data ());
  if (r)
    return r;
  for (int p = 0; p < npictures; p++)
    ctx->unpack_routes[fused[p] ? SCHRO_HIP_UNPACK_ROUTE_FUSED : SCHRO_HIP_UNPACK_ROUTE_TWO_PASS]++;
  return 0;
}

void
schro_hip_unpack_geometry (int values[SCHRO_HIP_UNPACK_GEOMETRY])
{
  int px, rows;
  unpack_tile_geometry (&px, &rows);
  values[0] = 16 * px;
  values[1] = rows;
  for (int f = 0; f < 7; f++)
    for (int b = 0; b < 2; b++) {
      int *v = values + 2 + 4 * (2 * f + b);
      iwt_fwd_tile_geometry (f, b ? 4 : 2, &v[0], &v[1]);
      iwt_fwd_tile_halo (f, b ? 4 : 2, &v[2], &v[3]);
    }
}

int
schro_hip_unpack_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_UNPACK_ROUTES], int reset)
{
  return read_routes ("unpack_routes", ctx, &SchroHipContext::unpack_routes, counts, reset);
}

}                               // extern "C"
