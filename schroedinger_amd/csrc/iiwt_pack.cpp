// iiwt_pack.cpp -- r05: the inverse wavelet and the packed copy-out of an intra picture as ONE call (SURVEY 8f N2:
// "fusing it ... is required for 10-bit v210 output in config 5").
//
// The reference's chain for a picture without references whose output format is v210 (BASELINE config 5: VC-2 low delay,
// 10-bit 4:2:2): x_wavelet_transform writes the pixel frame (s32 for > 8-bit streams, schrodecoder.c:1855-1886), x_combine
// converts it into the application's picture (schro_frame_convert, :2011-2052 -> schrovirtframe.c:1438-1537 convert_s16_s32,
// :1823-1895 crop / edge extend, :943-991 pack_v210_s16).  On the device that was two launches with the 4-byte pixel frame
// written and read back between them: per 8K picture 265 MB out + 265 MB in around 88 MB of v210.  The routes now
// (schro_hip_v210_routes counts the pictures of each):
//   HAAR3     the three-level s32 Haar of a 4:2:2 picture whose size is the transform's and a multiple of 192 x 8 (iiwt_haar.hip:
//             an 8 x 8 block of samples depends on 64 coefficients of its own 8 frame rows): the copy-out is the transform
//             kernel's epilogue.  Every picture of the call must allow it.
//   LEVEL     every other picture, every filter, depth and sample type: levels depth-1 .. 1 run through the level loop
//             (schro_hip_iiwt_batch on the frame's level-1 view) into compact LL planes -- a quarter of each component -- in
//             the queue's grow-only block, then ONE launch of iiwt_v210_kernel (iiwt.hip) for all pictures of the call lifts
//             the finest level of Y, U and V per tile and packs the v210 groups: the pixel frame is never written.  Depth 1
//             reads the LL band from the frame's LL quadrant.  Per 8K s32 DD(9,7) picture 0.173 against 0.266 ms.
//   TWO_PASS  the pixel frame in that block, then the pack, only where the level kernel cannot apply:
//               * dst or dst_stride not a multiple of 16 bytes (its stores are whole 16-byte v210 groups);
//               * a coefficient plane or stride not aligned to the sample size;
//               * dst overlapping a coefficient plane (the two passes read every coefficient before the pack writes);
//               * experiments library: SCHRO_HIP_V210_TWO_PASS=1 (A/B runs).
//             Every filter measured faster on LEVEL than on two passes (Fidelity too: 0.291 against 0.336 ms per 8K picture),
//             so no filter is sent to two passes; nor is a plane narrower than one tile (the tile clamps to the picture).
// The bytes out are the same on every route.
#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace schro;

extern "C" int
schro_hip_iiwt_pack_v210_batch (SchroHipContext * ctx, const SchroHipIwtPackPicture * pictures, int npictures, int depth, int filter,
    int bytes_per_sample)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && npictures > 0 && npictures <= kMaxJobs, "iiwt_pack_v210_batch: bad arguments");
  SCHRO_HIP_REQUIRE (depth >= 1 && depth <= 6 && filter >= 0 && filter <= 6 && (bytes_per_sample == 2 || bytes_per_sample == 4),
      "iiwt_pack_v210_batch: depth %d, filter %d, %d bytes per sample", depth, filter, bytes_per_sample);
  (void) hipSetDevice (ctx->device);
  bool fused = depth == 3 && (filter == 3 || filter == 4) && bytes_per_sample == 4;
  std::vector < HaarPackJob > jobs ((size_t) npictures);
  int tile_base = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipIwtPackPicture & pic = pictures[p];
    SCHRO_HIP_REQUIRE (pic.src[0] && pic.src[1] && pic.src[2] && pic.dst && pic.width > 0 && pic.height > 0
        && pic.out_width > 0 && pic.out_height > 0 && pic.out_width <= pic.width && pic.out_height <= pic.height
        && pic.dst_stride >= 16 * ((pic.out_width + 5) / 6), "iiwt_pack_v210_batch: picture %d: bad geometry", p);
    // (convert_4xx_422 of s16 / s32 frames is not on the reference's path either: schro_frame_convert finds no match, schroframe.c:869-979)
    SCHRO_HIP_REQUIRE (pic.h_shift == 1 && pic.v_shift == 0, "iiwt_pack_v210_batch: picture %d: v210 from s16 / s32 frames needs a 4:2:2 frame", p);
    // (what schro_hip_iiwt_batch asks of every component: whole transform levels, rows that hold the component)
    for (int c = 0; c < 3; c++) {
      const int w = c ? pic.width >> pic.h_shift : pic.width, h = c ? pic.height >> pic.v_shift : pic.height;
      SCHRO_HIP_REQUIRE (w % (1 << depth) == 0 && h % (1 << depth) == 0 && w > 0 && h > 0,
          "iiwt_pack_v210_batch: picture %d component %d: size %dx%d is not a multiple of 2^depth", p, c, w, h);
      SCHRO_HIP_REQUIRE (pic.src_stride[c] >= w * bytes_per_sample,
          "iiwt_pack_v210_batch: picture %d component %d: stride %d does not hold %d samples", p, c, pic.src_stride[c], w);
    }
    HaarPackJob & j = jobs[(size_t) p];
    for (int c = 0; c < 3; c++) {
      j.src[c] = pic.src[c];
      j.src_stride[c] = pic.src_stride[c];
    }
    j.w = pic.width;
    j.h = pic.height;
    j.dst = pic.dst;
    j.dst_stride = pic.dst_stride;
    j.tiles_x = div_up (pic.width, iiwt_haar3_v210_strip_width ());
    j.tile_base = tile_base;
    tile_base += j.tiles_x * (pic.height / 8);
    fused = fused && pic.h_shift == 1 && pic.v_shift == 0 && pic.out_width == pic.width && pic.out_height == pic.height
        && iiwt_haar3_v210_ok (j);
  }
  if (fused) {
    void *d_jobs;
    int r = push_args (ctx, jobs.data (), sizeof (HaarPackJob) * jobs.size (), &d_jobs);
    if (r)
      return r;
    ProfileScope ps (ctx, SCHRO_HIP_KERNEL_IIWT_FINEST);
    r = launch_iiwt_haar3_v210 (ctx->stream, (const HaarPackJob *) d_jobs, npictures, tile_base, filter);
    if (!r)
      ctx->v210_routes[SCHRO_HIP_V210_ROUTE_HAAR3] += npictures;
    return r;
  }
  // which pictures the finest level's v210 kernel takes (the rest: the two passes); a 16-byte aligned destination (its
  // stores are whole v210 groups), sample-aligned coefficient rows
  // (experiments: SCHRO_HIP_V210_TWO_PASS=1 sends every picture the Haar kernel does not take to the two passes, for A/B runs)
  const bool level_on = !(SCHRO_ENV ("SCHRO_HIP_V210_TWO_PASS") && atoi (SCHRO_ENV ("SCHRO_HIP_V210_TWO_PASS")) != 0);
  std::vector < char >level ((size_t) npictures, 0);
  int nlevel = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipIwtPackPicture & pic = pictures[p];
    uintptr_t src_bits = 0;
    bool apart = true;          // (the two passes read every coefficient before the pack writes dst; one launch does not)
    const char *d0 = (const char *) pic.dst, *d1 = d0 + (size_t) pic.dst_stride * pic.out_height;
    for (int c = 0; c < 3; c++) {
      src_bits |= (uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c];
      const char *s0 = (const char *) pic.src[c], *s1 = s0 + (size_t) pic.src_stride[c] * (c ? pic.height >> pic.v_shift : pic.height);
      apart = apart && (s1 <= d0 || d1 <= s0);
    }
    level[(size_t) p] = level_on && ((((uintptr_t) pic.dst | (uintptr_t) pic.dst_stride) & 15) == 0)
        && (src_bits & (bytes_per_sample - 1)) == 0 && apart;
    nlevel += level[(size_t) p];
  }
  // the queue's grow-only block: per level picture the three compact LL planes of level 0 (depth > 1: the coarser levels'
  // output, a quarter of the component), per two-pass picture its three pixel planes
  // r06: nothing is allocated, freed or waited for per call; a block that must grow waits for the queue once
  auto ll_stride = [&](int w) { return (int) round_up ((size_t) (w >> 1) * bytes_per_sample, 128); };
  size_t need = 0;
  for (int p = 0; p < npictures; p++)
    for (int c = 0; c < 3; c++) {
      const SchroHipIwtPackPicture & pic = pictures[p];
      const int w = c ? pic.width >> pic.h_shift : pic.width, h = c ? pic.height >> pic.v_shift : pic.height;
      if (!level[(size_t) p])
        need += round_up (round_up ((size_t) w * bytes_per_sample, 64) * (size_t) h, 256);
      else if (depth > 1)
        need += round_up ((size_t) ll_stride (w) * (size_t) (h >> 1), 256);
    }
  const int q = ctx->cur;
  if (ctx->pack_tmp_size_q[q] < need) {
    if (ctx->pack_tmp_q[q]) {
      SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
      SCHRO_HIP_CHECK (hipFree (ctx->pack_tmp_q[q]));
      ctx->pack_tmp_q[q] = nullptr;
      ctx->pack_tmp_size_q[q] = 0;
    }
    SCHRO_HIP_CHECK (hipMalloc (&ctx->pack_tmp_q[q], need));
    ctx->pack_tmp_size_q[q] = need;
  }
  size_t at = 0;
  int r = 0;

  // ---- the level route: levels depth-1 .. 1 by the level loop into the LL planes, then the finest level + v210 ----
  if (nlevel) {
    std::vector < SchroHipIwtPlane > coarse;
    std::vector < V210Job > vj;
    int cols, rows;
    iiwt_v210_geometry (filter, bytes_per_sample, &cols, &rows);
    const int vl = 8 / bytes_per_sample;
    int vtiles = 0;
    for (int p = 0; p < npictures; p++) {
      if (!level[(size_t) p])
        continue;
      const SchroHipIwtPackPicture & pic = pictures[p];
      V210Job j;
      memset (&j, 0, sizeof (j));
      for (int c = 0; c < 3; c++) {
        const int w = c ? pic.width >> pic.h_shift : pic.width, h = pic.height;
        j.src[c] = pic.src[c];
        j.src_stride[c] = pic.src_stride[c];
        if (depth > 1) {
          // the level-1 view of the coefficient frame {w / 2, h / 2, stride x 2} (schroparams.c:319-352), depth - 1 levels
          void *t = (char *) ctx->pack_tmp_q[q] + at;
          at += round_up ((size_t) ll_stride (w) * (size_t) (h >> 1), 256);
          SchroHipIwtPlane pl;
          memset (&pl, 0, sizeof (pl));
          pl.src = pic.src[c];
          pl.src_stride = 2 * pic.src_stride[c];
          pl.dst = t;
          pl.dst_stride = ll_stride (w);
          pl.width = w >> 1;
          pl.height = h >> 1;
          coarse.push_back (pl);
          j.ll[c] = t;
          j.ll_stride[c] = ll_stride (w);
        } else {
          j.ll[c] = pic.src[c];             // (the frame's LL quadrant)
          j.ll_stride[c] = 2 * pic.src_stride[c];
        }
        // 8-byte loads of the four bands: whole groups of samples per row, 8-byte aligned rows and band origins
        const int nc = w >> 1;
        const uintptr_t bits = (uintptr_t) j.ll[c] | (uintptr_t) j.ll_stride[c] | (uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c]
            | (uintptr_t) nc * bytes_per_sample;
        if (nc % vl == 0 && nc >= vl && (bits & 7) == 0)
          j.flags |= 1 << c;
      }
      j.w = pic.width;
      j.h = pic.height;
      j.out_w = pic.out_width;
      j.out_h = pic.out_height;
      j.dst = pic.dst;
      j.dst_stride = pic.dst_stride;
      j.tiles_x = div_up (pic.out_width, cols);
      j.tile_base = vtiles;
      vtiles += j.tiles_x * div_up (pic.out_height, rows);
      vj.push_back (j);
    }
    if (!coarse.empty ())
      r = schro_hip_iiwt_batch (ctx, coarse.data (), (int) coarse.size (), depth - 1, filter, bytes_per_sample);
    void *d_vj = nullptr;
    if (!r)
      r = push_args (ctx, vj.data (), sizeof (V210Job) * vj.size (), &d_vj);
    if (r)
      return r;
    {
      ProfileScope ps (ctx, SCHRO_HIP_KERNEL_IIWT_FINEST);
      r = launch_iiwt_v210 (ctx->stream, (const V210Job *) d_vj, (int) vj.size (), vtiles, filter, bytes_per_sample);
    }
    if (r)
      return r;
    ctx->v210_routes[SCHRO_HIP_V210_ROUTE_LEVEL] += nlevel;
    if (nlevel == npictures)
      return 0;
  }

  // ---- the two passes (the general form): transform into pixel planes, then the pack ----
  std::vector < SchroHipIwtPlane > planes;
  std::vector < SchroHipPackPlane > packs;
  for (int p = 0; p < npictures; p++) {
    if (level[(size_t) p])
      continue;
    const SchroHipIwtPackPicture & pic = pictures[p];
    SchroHipPackPlane pk;
    memset (&pk, 0, sizeof (pk));
    for (int c = 0; c < 3; c++) {
      const int w = c ? pic.width >> pic.h_shift : pic.width, h = c ? pic.height >> pic.v_shift : pic.height;
      const int stride = (int) round_up ((size_t) w * bytes_per_sample, 64);
      void *t = (char *) ctx->pack_tmp_q[q] + at;
      at += round_up ((size_t) stride * (size_t) h, 256);
      SchroHipIwtPlane pl;
      memset (&pl, 0, sizeof (pl));
      pl.src = pic.src[c];
      pl.src_stride = pic.src_stride[c];
      pl.dst = t;
      pl.dst_stride = stride;
      pl.width = w;
      pl.height = h;
      planes.push_back (pl);
      pk.src[c] = (const uint8_t *) t;
      pk.src_stride[c] = stride;
    }
    pk.src_width = pic.out_width;       // (the picture inside the transform's padded size: crop, schrovirtframe.c:1823-1853)
    pk.src_height = pic.out_height;
    pk.src_h_shift = pic.h_shift;
    pk.src_v_shift = pic.v_shift;
    pk.dst = pic.dst;
    pk.dst_stride = pic.dst_stride;
    pk.width = pic.out_width;
    pk.height = pic.out_height;
    pk.format = SCHRO_HIP_FORMAT_v210;
    packs.push_back (pk);
  }
  r = schro_hip_iiwt_batch (ctx, planes.data (), (int) planes.size (), depth, filter, bytes_per_sample);
  if (!r)
    r = schro_hip_pack_v210_batch (ctx, packs.data (), (int) packs.size (), bytes_per_sample);
  if (!r)
    ctx->v210_routes[SCHRO_HIP_V210_ROUTE_TWO_PASS] += (long long) packs.size ();
  return r;
}

extern "C" int
schro_hip_v210_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_V210_ROUTES], int reset)
{
  SCHRO_HIP_REQUIRE (ctx && counts, "v210_routes: bad arguments");
  for (int k = 0; k < SCHRO_HIP_V210_ROUTES; k++) {
    counts[k] = ctx->v210_routes[k];
    if (reset)
      ctx->v210_routes[k] = 0;
  }
  return 0;
}

// ---- 8-bit packed output: YUYV / UYVY / AYUV (schro_hip.h: schro_hip_iiwt_pack_u8_batch) ---------------------------
// The chain the call replaces for a picture that is not a reference: schro_hip_iiwt_batch in its combine form (the planar u8
// picture: + 128, or + the prediction), then schro_hip_pack_u8_batch -- 10 bytes per 4:2:2 pixel with a prediction where
// the coefficients, the prediction and the packed rows are 6.  Routes, per picture (schro_hip_pack8_routes):
//   LEVEL     s16, the source's chroma format the packed format's own, the alignments of the header: levels depth-1 .. 1
//             into compact LL planes in the queue's block, then ONE launch of iiwt_pack8_kernel (iiwt.hip) for all
//             such YUYV / UYVY pictures of the call and one for its AYUV pictures.
//   TWO_PASS  every other picture: the planar picture in the queue's block (one combine-form transform call for all of
//             them), then one pack launch.
//             Also the filters for which 8 x 2160p per call did NOT measure faster on LEVEL than on the chain by more
//             than the round-to-round spread, with and without a prediction (profiles/r09_pack8_fused.txt; below ms per
//             call with a prediction, level / chain): their chain ends in the register kernel's combine form, the level
//             route in the LDS tile.  4:2:2 -> YUYV / UYVY: DD(9,7) 0.216 / 0.193, LeGall 0.204 / 0.203, DD(13,7)
//             0.235 / 0.223, Daub(9,7) 0.304 / 0.227 keep the two passes (Haar 0.163 / 0.199 and Fidelity 0.423 / 0.719
//             take LEVEL); 4:4:4 -> AYUV: DD(9,7) 0.294 / 0.364 and DD(13,7) 0.339 / 0.403 (gains of 19 % and 16 %
//             inside the 20 % spread of their rounds) and Daub(9,7) 0.421 / 0.412 keep them (LeGall 0.277 / 0.384,
//             Haar 0.245 / 0.382, Fidelity 0.582 / 1.127 take LEVEL).
//             (experiments library: SCHRO_HIP_PACK8_TWO_PASS=1 sends every picture here, SCHRO_HIP_PACK8_LEVEL=1 lets
//             every filter take LEVEL, for A/B runs and the tests of those kernels.)
static bool
pack8_level_filter (int filter, bool ayuv)
{
  return ayuv ? (filter == 1 || (filter >= 3 && filter <= 5)) : (filter >= 3 && filter <= 5);
}

static bool
pack8_apart (const void *a, size_t an, const void *b, size_t bn)
{
  const char *a0 = (const char *) a, *b0 = (const char *) b;
  return a0 + an <= b0 || b0 + bn <= a0;
}

extern "C" int
schro_hip_iiwt_pack_u8_batch (SchroHipContext * ctx, const SchroHipIwtPack8Picture * pictures, int npictures, int depth, int filter,
    int bytes_per_sample)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && npictures > 0 && 3 * npictures <= kMaxJobs, "iiwt_pack_u8_batch: bad arguments");
  SCHRO_HIP_REQUIRE (depth >= 1 && depth <= 6 && filter >= 0 && filter <= 6 && (bytes_per_sample == 2 || bytes_per_sample == 4),
      "iiwt_pack_u8_batch: depth %d, filter %d, %d bytes per sample", depth, filter, bytes_per_sample);
  (void) hipSetDevice (ctx->device);
  const int bps = bytes_per_sample;
  const bool level_on = !(SCHRO_ENV ("SCHRO_HIP_PACK8_TWO_PASS") && atoi (SCHRO_ENV ("SCHRO_HIP_PACK8_TWO_PASS")) != 0);
  const bool level_all = SCHRO_ENV ("SCHRO_HIP_PACK8_LEVEL") && atoi (SCHRO_ENV ("SCHRO_HIP_PACK8_LEVEL")) != 0;
  auto comp_w = [](const SchroHipIwtPack8Picture & pic, int c, int w) { return c ? (w + pic.h_shift) >> pic.h_shift : w; };
  auto comp_h = [](const SchroHipIwtPack8Picture & pic, int c, int h) { return c ? (h + pic.v_shift) >> pic.v_shift : h; };
  std::vector < char >level ((size_t) npictures, 0);
  int nlevel = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipIwtPack8Picture & pic = pictures[p];
    SCHRO_HIP_REQUIRE (pic.format == SCHRO_HIP_FORMAT_YUYV || pic.format == SCHRO_HIP_FORMAT_UYVY || pic.format == SCHRO_HIP_FORMAT_AYUV,
        "iiwt_pack_u8_batch: picture %d: format 0x%x is not YUYV / UYVY / AYUV", p, pic.format);
    const bool ayuv = pic.format == SCHRO_HIP_FORMAT_AYUV;
    SCHRO_HIP_REQUIRE (pic.src[0] && pic.src[1] && pic.src[2] && pic.dst && pic.width > 0 && pic.height > 0
        && pic.out_width > 0 && pic.out_height > 0 && pic.out_width <= pic.width && pic.out_height <= pic.height
        && pic.dst_stride >= (ayuv ? 4 * pic.out_width : 4 * (pic.out_width / 2)), "iiwt_pack_u8_batch: picture %d: bad geometry", p);
    SCHRO_HIP_REQUIRE ((pic.h_shift == 0 || pic.h_shift == 1) && (pic.v_shift == 0 || pic.v_shift == 1) && !(pic.v_shift && !pic.h_shift),
        "iiwt_pack_u8_batch: picture %d: chroma format not 4:4:4 / 4:2:2 / 4:2:0", p);
    const bool has_pred = pic.pred[0] != nullptr;
    SCHRO_HIP_REQUIRE ((pic.pred[1] != nullptr) == has_pred && (pic.pred[2] != nullptr) == has_pred,
        "iiwt_pack_u8_batch: picture %d: a prediction for some components and not for others", p);
    bool fits = bps == 2 && level_on && (level_all || pack8_level_filter (filter, ayuv)) && pic.v_shift == 0 && pic.h_shift == (ayuv ? 0 : 1)
        && ((((uintptr_t) pic.dst | (uintptr_t) pic.dst_stride) & 15) == 0);
    const size_t dst_bytes = (size_t) pic.dst_stride * pic.out_height;
    for (int c = 0; c < 3; c++) {
      // (what schro_hip_iiwt_batch asks of every component: whole transform levels, rows that hold the component)
      const int w = c ? pic.width >> pic.h_shift : pic.width, h = c ? pic.height >> pic.v_shift : pic.height;
      SCHRO_HIP_REQUIRE (w % (1 << depth) == 0 && h % (1 << depth) == 0 && w > 0 && h > 0 && (w << (c ? pic.h_shift : 0)) == pic.width
          && (h << (c ? pic.v_shift : 0)) == pic.height,
          "iiwt_pack_u8_batch: picture %d component %d: size %dx%d is not a multiple of 2^depth", p, c, w, h);
      SCHRO_HIP_REQUIRE (pic.src_stride[c] >= w * bps,
          "iiwt_pack_u8_batch: picture %d component %d: stride %d does not hold %d samples", p, c, pic.src_stride[c], w);
      const int ow = comp_w (pic, c, pic.out_width), oh = comp_h (pic, c, pic.out_height);
      SCHRO_HIP_REQUIRE (!has_pred || pic.pred_stride[c] >= ow,
          "iiwt_pack_u8_batch: picture %d component %d: prediction stride %d does not hold %d samples", p, c, pic.pred_stride[c], ow);
      fits = fits && ((((uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c]) & (bps - 1)) == 0)
          && pack8_apart (pic.dst, dst_bytes, pic.src[c], (size_t) pic.src_stride[c] * h);
      if (has_pred)
        fits = fits && ((((uintptr_t) pic.pred[c] | (uintptr_t) pic.pred_stride[c]) & 7) == 0) && pic.pred_stride[c] >= ((ow + 7) & ~7)
            && pack8_apart (pic.dst, dst_bytes, pic.pred[c], (size_t) pic.pred_stride[c] * oh);
    }
    level[(size_t) p] = fits;
    nlevel += fits;
  }
  // the queue's grow-only block (shared with the v210 call: in-order reuse on the queue): per level picture the three
  // compact LL planes of level 0 (depth > 1), per two-pass picture its three u8 planes
  auto ll_stride = [&](int w) { return (int) round_up ((size_t) (w >> 1) * bps, 128); };
  size_t need = 0;
  for (int p = 0; p < npictures; p++)
    for (int c = 0; c < 3; c++) {
      const SchroHipIwtPack8Picture & pic = pictures[p];
      if (!level[(size_t) p])
        need += round_up (round_up ((size_t) comp_w (pic, c, pic.out_width), 64) * (size_t) comp_h (pic, c, pic.out_height), 256);
      else if (depth > 1)
        need += round_up ((size_t) ll_stride (c ? pic.width >> pic.h_shift : pic.width) * (size_t) (pic.height >> 1), 256);
    }
  const int q = ctx->cur;
  if (ctx->pack_tmp_size_q[q] < need) {
    if (ctx->pack_tmp_q[q]) {
      SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
      SCHRO_HIP_CHECK (hipFree (ctx->pack_tmp_q[q]));
      ctx->pack_tmp_q[q] = nullptr;
      ctx->pack_tmp_size_q[q] = 0;
    }
    SCHRO_HIP_CHECK (hipMalloc (&ctx->pack_tmp_q[q], need));
    ctx->pack_tmp_size_q[q] = need;
  }
  size_t at = 0;
  int r = 0;

  // ---- the level route: levels depth-1 .. 1 by the level loop into the LL planes, then the finest level + pack ----
  if (nlevel) {
    std::vector < SchroHipIwtPlane > coarse;
    std::vector < Pack8Job > pj[2];     // [0] YUYV / UYVY, [1] AYUV: one launch each
    int tiles[2] = { 0, 0 };
    for (int p = 0; p < npictures; p++) {
      if (!level[(size_t) p])
        continue;
      const SchroHipIwtPack8Picture & pic = pictures[p];
      const int ayuv = pic.format == SCHRO_HIP_FORMAT_AYUV;
      int cols, rows;
      iiwt_pack8_geometry (filter, ayuv, &cols, &rows);
      Pack8Job j;
      memset (&j, 0, sizeof (j));
      for (int c = 0; c < 3; c++) {
        const int w = c ? pic.width >> pic.h_shift : pic.width, h = pic.height;
        j.src[c] = pic.src[c];
        j.src_stride[c] = pic.src_stride[c];
        j.pred[c] = pic.pred[c];
        j.pred_stride[c] = pic.pred_stride[c];
        if (depth > 1) {
          // the level-1 view of the coefficient frame {w / 2, h / 2, stride x 2} (schroparams.c:319-352), depth - 1 levels
          void *t = (char *) ctx->pack_tmp_q[q] + at;
          at += round_up ((size_t) ll_stride (w) * (size_t) (h >> 1), 256);
          SchroHipIwtPlane pl;
          memset (&pl, 0, sizeof (pl));
          pl.src = pic.src[c];
          pl.src_stride = 2 * pic.src_stride[c];
          pl.dst = t;
          pl.dst_stride = ll_stride (w);
          pl.width = w >> 1;
          pl.height = h >> 1;
          coarse.push_back (pl);
          j.ll[c] = t;
          j.ll_stride[c] = ll_stride (w);
        } else {
          j.ll[c] = pic.src[c];             // (the frame's LL quadrant)
          j.ll_stride[c] = 2 * pic.src_stride[c];
        }
        // 8-byte loads of the four bands: whole groups of samples per row, 8-byte aligned rows and band origins
        const int nc = w >> 1, vl = 8 / bps;
        const uintptr_t bits = (uintptr_t) j.ll[c] | (uintptr_t) j.ll_stride[c] | (uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c]
            | (uintptr_t) nc * bps;
        if (nc % vl == 0 && nc >= vl && (bits & 7) == 0)
          j.flags |= 1 << c;
      }
      if (pic.format == SCHRO_HIP_FORMAT_UYVY)
        j.flags |= 8;
      j.w = pic.width;
      j.h = pic.height;
      j.out_w = pic.out_width;
      j.out_h = pic.out_height;
      j.dst = pic.dst;
      j.dst_stride = pic.dst_stride;
      j.tiles_x = div_up (pic.out_width, cols);
      j.tile_base = tiles[ayuv];
      tiles[ayuv] += j.tiles_x * div_up (pic.out_height, rows);
      pj[ayuv].push_back (j);
    }
    if (!coarse.empty ())
      r = schro_hip_iiwt_batch (ctx, coarse.data (), (int) coarse.size (), depth - 1, filter, bps);
    for (int ayuv = 0; ayuv < 2 && !r; ayuv++) {
      if (pj[ayuv].empty ())
        continue;
      void *d_pj = nullptr;
      r = push_args (ctx, pj[ayuv].data (), sizeof (Pack8Job) * pj[ayuv].size (), &d_pj);
      if (r)
        break;
      ProfileScope ps (ctx, SCHRO_HIP_KERNEL_IIWT_FINEST);
      r = launch_iiwt_pack8 (ctx->stream, (const Pack8Job *) d_pj, (int) pj[ayuv].size (), tiles[ayuv], filter, ayuv);
    }
    if (r)
      return r;
    ctx->pack8_routes[SCHRO_HIP_PACK8_ROUTE_LEVEL] += nlevel;
    if (nlevel == npictures)
      return 0;
  }

  // ---- the two passes (the general form): the combine form into planar u8 planes, then the pack ----
  std::vector < SchroHipIwtPlane > planes;
  std::vector < SchroHipPackPlane > packs;
  for (int p = 0; p < npictures; p++) {
    if (level[(size_t) p])
      continue;
    const SchroHipIwtPack8Picture & pic = pictures[p];
    SchroHipPackPlane pk;
    memset (&pk, 0, sizeof (pk));
    for (int c = 0; c < 3; c++) {
      const int ow = comp_w (pic, c, pic.out_width), oh = comp_h (pic, c, pic.out_height);
      const int stride = (int) round_up ((size_t) ow, 64);
      void *t = (char *) ctx->pack_tmp_q[q] + at;
      at += round_up ((size_t) stride * (size_t) oh, 256);
      SchroHipIwtPlane pl;
      memset (&pl, 0, sizeof (pl));
      pl.src = pic.src[c];
      pl.src_stride = pic.src_stride[c];
      pl.dst = t;
      pl.dst_stride = stride;
      pl.width = c ? pic.width >> pic.h_shift : pic.width;
      pl.height = c ? pic.height >> pic.v_shift : pic.height;
      pl.combine = pic.pred[0] ? 1 : 2;
      pl.pred = pic.pred[c];
      pl.pred_stride = pic.pred_stride[c];
      pl.out_width = ow;
      pl.out_height = oh;
      planes.push_back (pl);
      pk.src[c] = (const uint8_t *) t;
      pk.src_stride[c] = stride;
    }
    pk.src_width = pic.out_width;
    pk.src_height = pic.out_height;
    pk.src_h_shift = pic.h_shift;
    pk.src_v_shift = pic.v_shift;
    pk.dst = pic.dst;
    pk.dst_stride = pic.dst_stride;
    pk.width = pic.out_width;
    pk.height = pic.out_height;
    pk.format = pic.format;
    packs.push_back (pk);
  }
  r = schro_hip_iiwt_batch (ctx, planes.data (), (int) planes.size (), depth, filter, bps);
  if (!r)
    r = schro_hip_pack_u8_batch (ctx, packs.data (), (int) packs.size ());
  if (!r)
    ctx->pack8_routes[SCHRO_HIP_PACK8_ROUTE_TWO_PASS] += (long long) packs.size ();
  return r;
}

extern "C" int
schro_hip_pack8_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_PACK8_ROUTES], int reset)
{
  SCHRO_HIP_REQUIRE (ctx && counts, "pack8_routes: bad arguments");
  for (int k = 0; k < SCHRO_HIP_PACK8_ROUTES; k++) {
    counts[k] = ctx->pack8_routes[k];
    if (reset)
      ctx->pack8_routes[k] = 0;
  }
  return 0;
}

// ---- > 8-bit packed output: v216 / ARGB / AY64 (schro_hip.h: schro_hip_iiwt_pack_wide_batch) -----------------------
// The chain the call replaces -- the non-reference intra tail of x_combine for a > 8-bit picture (schrodecoder.c:2009-2021):
// schro_hip_iiwt_batch into s16 / s32 pixel planes, schro_hip_shift_right_batch where shift != 0, schro_hip_pack_wide_batch.
// Per 4:4:4 s32 pixel into AY64 that is 12 + 12 (+ 12 + 12 with a shift) + 12 + 8 bytes of memory traffic where the
// coefficients and the packed rows are 12 + 8.  Routes, per picture (schro_hip_wide_routes):
//   LEVEL     levels depth-1 .. 1 into compact LL planes in the queue's block, then ONE launch of iiwt_wide_kernel
//             (iiwt.hip) for all such v216 pictures of the call and one for its ARGB / AY64 pictures: the sink shifts and
//             converts, the lanes write whole packed groups.
//   TWO_PASS  the pixel planes in the queue's block (one transform call for all such pictures), one shift launch per
//             distinct shift, one pack launch: a dst or dst_stride that is not a multiple of 16, coefficient planes not
//             aligned to their sample size, a dst that overlaps a coefficient plane, a v216 row without a pixel pair --
//             and the combinations wide_level_combination () names.
//             (experiments library: SCHRO_HIP_WIDE_TWO_PASS=1 sends every picture here, SCHRO_HIP_WIDE_LEVEL=1 lets every
//             combination take LEVEL, for A/B runs and the tests of those kernels.)
// The rule of which format x filter x sample type takes LEVEL: only where scripts/wide_fused_ab.py measured LEVEL faster
// than the chain by more than the larger of the two forms' spreads, without a shift AND with one
// (profiles/r10_wide_fused.txt: depth 3, 8 x 2160p per call and one 8K picture for v216; ms per call, level / chain, without a
// shift -- with a shift the chain pays its shift launch as well and every combination is 2 to 5 times faster on LEVEL):
//   s32, every format and filter: v216 0.179 / 0.353 (Haar) .. 0.360 / 0.618 (Fidelity), 8K 0.127 / 0.248 (DD(9,7));
//        ARGB 0.295 / 0.548 (Haar) .. 0.771 / 0.939 (Fidelity, the narrowest: 18 % against spreads of 5 %);
//        AY64 0.333 / 0.550 (Haar) .. 0.777 / 0.939 (Fidelity).  Their chain has no register kernel.
//   s16 -> v216, every filter: 0.132 / 0.267 (Haar) .. 0.189 / 0.280 (Daub(9,7)); the luma columns pack_v216 never reads
//        are not lifted at the finest level.
//   s16 -> ARGB: DD(9,7) 0.292 / 0.359, LeGall 0.299 / 0.383, Haar 0.223 / 0.383 take LEVEL; DD(13,7) 0.346 / 0.397 and
//        Fidelity 0.643 / 0.702 won inside a spread of 18 % and 15 %, Daub(9,7) 0.430 / 0.401 lost: the two passes, whose
//        transform ends in the register kernel (what r09 found for the 8-bit formats).
//   s16 -> AY64: every filter (DD(9,7) 0.319 / 0.452 .. Fidelity 0.648 / 0.794) but Daub(9,7), 0.436 / 0.490 inside a
//        spread of 21 %.
static bool
wide_level_combination (int format, int filter, int bps)
{
  if (bps == 4 || format == SCHRO_HIP_FORMAT_v216)
    return true;
  if (format == SCHRO_HIP_FORMAT_ARGB)
    return filter == 0 || filter == 1 || filter == 3 || filter == 4;
  return filter != 6;
}

extern "C" int
schro_hip_iiwt_pack_wide_batch (SchroHipContext * ctx, const SchroHipIwtPackWidePicture * pictures, int npictures, int depth, int filter,
    int bytes_per_sample)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && npictures > 0 && 3 * npictures <= kMaxJobs, "iiwt_pack_wide_batch: bad arguments");
  SCHRO_HIP_REQUIRE (depth >= 1 && depth <= 6 && filter >= 0 && filter <= 6 && (bytes_per_sample == 2 || bytes_per_sample == 4),
      "iiwt_pack_wide_batch: depth %d, filter %d, %d bytes per sample", depth, filter, bytes_per_sample);
  (void) hipSetDevice (ctx->device);
  const int bps = bytes_per_sample;
  const bool level_on = !(SCHRO_ENV ("SCHRO_HIP_WIDE_TWO_PASS") && atoi (SCHRO_ENV ("SCHRO_HIP_WIDE_TWO_PASS")) != 0);
  const bool level_all = SCHRO_ENV ("SCHRO_HIP_WIDE_LEVEL") && atoi (SCHRO_ENV ("SCHRO_HIP_WIDE_LEVEL")) != 0;
  std::vector < char >level ((size_t) npictures, 0);
  int nlevel = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipIwtPackWidePicture & pic = pictures[p];
    SCHRO_HIP_REQUIRE (is_wide_format (pic.format), "iiwt_pack_wide_batch: picture %d: format 0x%x is not v216 / ARGB / AY64", p, pic.format);
    const bool v216 = pic.format == SCHRO_HIP_FORMAT_v216;
    const int row_bytes = v216 ? 8 * (pic.out_width / 2) : pic.format == SCHRO_HIP_FORMAT_ARGB ? 4 * pic.out_width : 8 * pic.out_width;
    SCHRO_HIP_REQUIRE (pic.src[0] && pic.src[1] && pic.src[2] && pic.dst && pic.width > 0 && pic.height > 0
        && pic.out_width > 0 && pic.out_height > 0 && pic.out_width <= pic.width && pic.out_height <= pic.height
        && pic.dst_stride >= row_bytes, "iiwt_pack_wide_batch: picture %d: bad geometry", p);
    // (no chroma resampling of s16 / s32 frames on the reference's path: as schro_hip_pack_wide_batch)
    SCHRO_HIP_REQUIRE (pic.v_shift == 0 && pic.h_shift == (v216 ? 1 : 0), "iiwt_pack_wide_batch: picture %d: the source must be %s", p,
        v216 ? "4:2:2" : "4:4:4");
    SCHRO_HIP_REQUIRE (pic.shift >= 0 && pic.shift < 8 * bps, "iiwt_pack_wide_batch: picture %d: shift %d", p, pic.shift);
    bool fits = level_on && (level_all || wide_level_combination (pic.format, filter, bps)) && row_bytes > 0
        && ((((uintptr_t) pic.dst | (uintptr_t) pic.dst_stride) & 15) == 0);
    const size_t dst_bytes = (size_t) pic.dst_stride * pic.out_height;
    for (int c = 0; c < 3; c++) {
      // (what schro_hip_iiwt_batch asks of every component: whole transform levels, rows that hold the component)
      const int w = c ? pic.width >> pic.h_shift : pic.width, h = pic.height;
      SCHRO_HIP_REQUIRE (w % (1 << depth) == 0 && h % (1 << depth) == 0 && w > 0 && (w << (c ? pic.h_shift : 0)) == pic.width,
          "iiwt_pack_wide_batch: picture %d component %d: size %dx%d is not a multiple of 2^depth", p, c, w, h);
      SCHRO_HIP_REQUIRE (pic.src_stride[c] >= w * bps,
          "iiwt_pack_wide_batch: picture %d component %d: stride %d does not hold %d samples", p, c, pic.src_stride[c], w);
      fits = fits && ((((uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c]) & (bps - 1)) == 0)
          && pack8_apart (pic.dst, dst_bytes, pic.src[c], (size_t) pic.src_stride[c] * h);
    }
    level[(size_t) p] = fits;
    nlevel += fits;
  }
  // the queue's grow-only block (shared with the v210 and the 8-bit calls: in-order reuse on the queue): per level picture
  // the three compact LL planes of level 0 (depth > 1), per two-pass picture its three pixel planes
  auto ll_stride = [&](int w) { return (int) round_up ((size_t) (w >> 1) * bps, 128); };
  size_t need = 0;
  for (int p = 0; p < npictures; p++)
    for (int c = 0; c < 3; c++) {
      const SchroHipIwtPackWidePicture & pic = pictures[p];
      const int w = c ? pic.width >> pic.h_shift : pic.width, h = pic.height;
      if (!level[(size_t) p])
        need += round_up (round_up ((size_t) w * bps, 64) * (size_t) h, 256);
      else if (depth > 1)
        need += round_up ((size_t) ll_stride (w) * (size_t) (h >> 1), 256);
    }
  const int q = ctx->cur;
  if (ctx->pack_tmp_size_q[q] < need) {
    if (ctx->pack_tmp_q[q]) {
      SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
      SCHRO_HIP_CHECK (hipFree (ctx->pack_tmp_q[q]));
      ctx->pack_tmp_q[q] = nullptr;
      ctx->pack_tmp_size_q[q] = 0;
    }
    SCHRO_HIP_CHECK (hipMalloc (&ctx->pack_tmp_q[q], need));
    ctx->pack_tmp_size_q[q] = need;
  }
  size_t at = 0;
  int r = 0;

  // ---- the level route: levels depth-1 .. 1 by the level loop into the LL planes, then the finest level + pack ----
  if (nlevel) {
    std::vector < SchroHipIwtPlane > coarse;
    std::vector < WideJob > wj[2];      // [0] ARGB / AY64, [1] v216: one launch each
    int tiles[2] = { 0, 0 };
    for (int p = 0; p < npictures; p++) {
      if (!level[(size_t) p])
        continue;
      const SchroHipIwtPackWidePicture & pic = pictures[p];
      const int v216 = pic.format == SCHRO_HIP_FORMAT_v216;
      int cols, rows;
      iiwt_wide_geometry (filter, v216, &cols, &rows);
      WideJob j;
      memset (&j, 0, sizeof (j));
      for (int c = 0; c < 3; c++) {
        const int w = c ? pic.width >> pic.h_shift : pic.width, h = pic.height;
        j.src[c] = pic.src[c];
        j.src_stride[c] = pic.src_stride[c];
        if (depth > 1) {
          // the level-1 view of the coefficient frame {w / 2, h / 2, stride x 2} (schroparams.c:319-352), depth - 1 levels
          void *t = (char *) ctx->pack_tmp_q[q] + at;
          at += round_up ((size_t) ll_stride (w) * (size_t) (h >> 1), 256);
          SchroHipIwtPlane pl;
          memset (&pl, 0, sizeof (pl));
          pl.src = pic.src[c];
          pl.src_stride = 2 * pic.src_stride[c];
          pl.dst = t;
          pl.dst_stride = ll_stride (w);
          pl.width = w >> 1;
          pl.height = h >> 1;
          coarse.push_back (pl);
          j.ll[c] = t;
          j.ll_stride[c] = ll_stride (w);
        } else {
          j.ll[c] = pic.src[c];             // (the frame's LL quadrant)
          j.ll_stride[c] = 2 * pic.src_stride[c];
        }
        // 8-byte loads of the four bands: whole groups of samples per row, 8-byte aligned rows and band origins
        const int nc = w >> 1, vl = 8 / bps;
        const uintptr_t bits = (uintptr_t) j.ll[c] | (uintptr_t) j.ll_stride[c] | (uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c]
            | (uintptr_t) nc * bps;
        if (nc % vl == 0 && nc >= vl && (bits & 7) == 0)
          j.flags |= 1 << c;
      }
      if (pic.format == SCHRO_HIP_FORMAT_AY64)
        j.flags |= 8;
      j.w = pic.width;
      j.h = pic.height;
      j.out_w = pic.out_width;
      j.out_h = pic.out_height;
      j.dst = pic.dst;
      j.dst_stride = pic.dst_stride;
      j.shift = pic.shift;
      // (v216: a tile is `cols` output pairs = luma columns; the luma columns from out_width / 2 on are never lifted)
      j.tiles_x = div_up (v216 ? pic.out_width / 2 : pic.out_width, cols);
      j.tile_base = tiles[v216];
      tiles[v216] += j.tiles_x * div_up (pic.out_height, rows);
      wj[v216].push_back (j);
    }
    if (!coarse.empty ())
      r = schro_hip_iiwt_batch (ctx, coarse.data (), (int) coarse.size (), depth - 1, filter, bps);
    for (int v216 = 0; v216 < 2 && !r; v216++) {
      if (wj[v216].empty ())
        continue;
      void *d_wj = nullptr;
      r = push_args (ctx, wj[v216].data (), sizeof (WideJob) * wj[v216].size (), &d_wj);
      if (r)
        break;
      ProfileScope ps (ctx, SCHRO_HIP_KERNEL_IIWT_FINEST);
      r = launch_iiwt_wide (ctx->stream, (const WideJob *) d_wj, (int) wj[v216].size (), tiles[v216], filter, bps, v216);
    }
    if (r)
      return r;
    ctx->wide_routes[SCHRO_HIP_WIDE_ROUTE_LEVEL] += nlevel;
    if (nlevel == npictures)
      return 0;
  }

  // ---- the two passes (the general form): transform into pixel planes, the shift, then the pack ----
  std::vector < SchroHipIwtPlane > planes;
  std::vector < SchroHipPackPlane > packs;
  std::vector < int >shifts;            // the distinct non-zero shifts of the call
  for (int p = 0; p < npictures; p++) {
    if (level[(size_t) p])
      continue;
    const SchroHipIwtPackWidePicture & pic = pictures[p];
    SchroHipPackPlane pk;
    memset (&pk, 0, sizeof (pk));
    for (int c = 0; c < 3; c++) {
      const int w = c ? pic.width >> pic.h_shift : pic.width, h = pic.height;
      const int stride = (int) round_up ((size_t) w * bps, 64);
      void *t = (char *) ctx->pack_tmp_q[q] + at;
      at += round_up ((size_t) stride * (size_t) h, 256);
      SchroHipIwtPlane pl;
      memset (&pl, 0, sizeof (pl));
      pl.src = pic.src[c];
      pl.src_stride = pic.src_stride[c];
      pl.dst = t;
      pl.dst_stride = stride;
      pl.width = w;
      pl.height = h;
      planes.push_back (pl);
      pk.src[c] = (const uint8_t *) t;
      pk.src_stride[c] = stride;
    }
    pk.src_width = pic.out_width;       // (the picture inside the transform's padded size: crop, schrovirtframe.c:1823-1853)
    pk.src_height = pic.out_height;
    pk.src_h_shift = pic.h_shift;
    pk.src_v_shift = pic.v_shift;
    pk.dst = pic.dst;
    pk.dst_stride = pic.dst_stride;
    pk.width = pic.out_width;
    pk.height = pic.out_height;
    pk.format = pic.format;
    packs.push_back (pk);
    bool seen = pic.shift == 0;
    for (int s : shifts)
      seen = seen || s == pic.shift;
    if (!seen)
      shifts.push_back (pic.shift);
  }
  r = schro_hip_iiwt_batch (ctx, planes.data (), (int) planes.size (), depth, filter, bps);
  for (size_t n = 0; n < shifts.size () && !r; n++) {
    // schro_frame_shift_right on the picture inside each plane (all the packer reads), one launch per distinct shift
    std::vector < SchroHipDcPlane > sp;
    size_t k = 0;
    for (int p = 0; p < npictures; p++) {
      if (level[(size_t) p])
        continue;
      const SchroHipIwtPackWidePicture & pic = pictures[p];
      for (int c = 0; c < 3; c++, k++) {
        if (pic.shift != shifts[n])
          continue;
        SchroHipDcPlane d;
        d.data = planes[k].dst;
        d.stride = planes[k].dst_stride;
        d.width = c ? (pic.out_width + pic.h_shift) >> pic.h_shift : pic.out_width;
        d.height = pic.out_height;
        sp.push_back (d);
      }
    }
    r = schro_hip_shift_right_batch (ctx, sp.data (), (int) sp.size (), bps, shifts[n]);
  }
  if (!r)
    r = schro_hip_pack_wide_batch (ctx, packs.data (), (int) packs.size (), bps);
  if (!r)
    ctx->wide_routes[SCHRO_HIP_WIDE_ROUTE_TWO_PASS] += (long long) packs.size ();
  return r;
}

extern "C" int
schro_hip_wide_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_WIDE_ROUTES], int reset)
{
  SCHRO_HIP_REQUIRE (ctx && counts, "wide_routes: bad arguments");
  for (int k = 0; k < SCHRO_HIP_WIDE_ROUTES; k++) {
    counts[k] = ctx->wide_routes[k];
    if (reset)
      ctx->wide_routes[k] = 0;
  }
  return 0;
}
