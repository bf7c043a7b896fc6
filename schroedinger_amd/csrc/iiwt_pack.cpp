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
//
// The 8-bit (YUYV / UYVY / AYUV) and the > 8-bit (v216 / ARGB / AY64) calls below have the LEVEL and TWO_PASS routes too.
// What the three share exists once, in front of them: the refusals, what LEVEL asks of every picture, the layout of the
// queue's block, the fields the three level jobs have in common, a TWO_PASS picture's planes.  None of it knows which call
// it serves: what differs comes in as an argument or stays with its call.
#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace schro;

// A plane of the queue's block
struct Slot {
  size_t at;
  int stride;
};

// The fields the three calls' pictures have in common, and what a call decided about the picture
struct PackPic {
  const void *src[3];
  int src_stride[3];
  int width, height, h_shift, v_shift;
  uint8_t *dst;
  int dst_stride;
  int out_width, out_height;
  bool level;                   // its route: LEVEL, else TWO_PASS
  int px_row_bytes[3], px_rows[3];      // the planes a TWO_PASS picture's transform writes and its pack reads
  Slot slot[3];                 // LEVEL (depth > 1): its compact LL planes; TWO_PASS: those planes

  int cw (int c) const { return c ? width >> h_shift : width; }
  int ch (int c) const { return c ? height >> v_shift : height; }
};

template < class Picture > static PackPic
common_fields (const Picture & pic)
{
  PackPic k;
  memset (&k, 0, sizeof (k));
  for (int c = 0; c < 3; c++) {
    k.src[c] = pic.src[c];
    k.src_stride[c] = pic.src_stride[c];
  }
  k.width = pic.width;
  k.height = pic.height;
  k.h_shift = pic.h_shift;
  k.v_shift = pic.v_shift;
  k.dst = pic.dst;
  k.dst_stride = pic.dst_stride;
  k.out_width = pic.out_width;
  k.out_height = pic.out_height;
  return k;
}

static bool
env_on (const char *value)
{
  return value && atoi (value) != 0;
}

// ---- the refusals (who: the call's name, as in motion_check_*) ------------------------------------------------------
static int
check_call (const char *who, const void *ctx, const void *pictures, int npictures, int njobs, int depth, int filter, int bps)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && npictures > 0 && njobs <= kMaxJobs, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (depth >= 1 && depth <= 6 && filter >= 0 && filter <= 6 && (bps == 2 || bps == 4),
      "%s: depth %d, filter %d, %d bytes per sample", who, depth, filter, bps);
  return 0;
}

static int
check_geometry (const char *who, int p, const PackPic & pic, int row_bytes)
{
  SCHRO_HIP_REQUIRE (pic.src[0] && pic.src[1] && pic.src[2] && pic.dst && pic.width > 0 && pic.height > 0
      && pic.out_width > 0 && pic.out_height > 0 && pic.out_width <= pic.width && pic.out_height <= pic.height
      && pic.dst_stride >= row_bytes, "%s: picture %d: bad geometry", who, p);
  return 0;
}

// What schro_hip_iiwt_batch asks of every component: whole transform levels, rows that hold the component.  (Behind the
// call's own check of h_shift and v_shift.  The v210 call's source is 4:2:2, and the wide call's v_shift is 0: there the
// terms that compare the shifted size with the picture's cannot fire, for luma is refused first and its width is even at
// depth >= 1.)
static int
check_component (const char *who, int p, int c, const PackPic & pic, int depth, int bps)
{
  const int w = pic.cw (c), h = pic.ch (c);
  SCHRO_HIP_REQUIRE (w % (1 << depth) == 0 && h % (1 << depth) == 0 && w > 0 && h > 0 && (w << (c ? pic.h_shift : 0)) == pic.width
      && (h << (c ? pic.v_shift : 0)) == pic.height, "%s: picture %d component %d: size %dx%d is not a multiple of 2^depth", who, p, c, w, h);
  SCHRO_HIP_REQUIRE (pic.src_stride[c] >= w * bps, "%s: picture %d component %d: stride %d does not hold %d samples", who, p, c,
      pic.src_stride[c], w);
  return 0;
}

// ---- the LEVEL route ------------------------------------------------------------------------------------------------
static bool
apart (const void *a, size_t an, const void *b, size_t bn)
{
  const char *a0 = (const char *) a, *b0 = (const char *) b;
  return a0 + an <= b0 || b0 + bn <= a0;
}

// What the finest level's kernels ask of every picture, whatever they pack: a 16-byte aligned destination (their stores
// are whole 16-byte groups), sample-aligned coefficient rows, a dst apart from every coefficient plane (the two passes
// read every coefficient before the pack writes dst; one launch does not)
static bool
level_fits (const PackPic & pic, int bps)
{
  bool fits = (((uintptr_t) pic.dst | (uintptr_t) pic.dst_stride) & 15) == 0;
  for (int c = 0; c < 3; c++)
    fits = fits && ((((uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c]) & (bps - 1)) == 0)
        && apart (pic.dst, (size_t) pic.dst_stride * pic.out_height, pic.src[c], (size_t) pic.src_stride[c] * pic.ch (c));
  return fits;
}

// The queue's grow-only block for one call (the three calls share it: in-order reuse on the queue): the LEVEL pictures
// first -- per picture the three compact LL planes of level 0 (depth > 1: the coarser levels' output, a quarter of the
// component) --, then per TWO_PASS picture its three planes.  What takes a plane moves the block's end, so the size is
// the end of the last plane.
// r06: nothing is allocated, freed or waited for per call; a block that must grow waits for the queue once
static int
lay_out_block (SchroHipContext * ctx, std::vector < PackPic > &pics, int depth, int bps, char **block)
{
  size_t end = 0;
  auto take = [&end] (size_t row_bytes, size_t row_align, int rows) {
    const Slot s = { end, (int) round_up (row_bytes, row_align) };
    end += round_up ((size_t) s.stride * (size_t) rows, 256);
    return s;
  };
  for (PackPic & pic : pics)
    for (int c = 0; c < 3 && pic.level && depth > 1; c++)
      pic.slot[c] = take ((size_t) (pic.cw (c) >> 1) * bps, 128, pic.ch (c) >> 1);
  for (PackPic & pic : pics)
    for (int c = 0; c < 3 && !pic.level; c++)
      pic.slot[c] = take ((size_t) pic.px_row_bytes[c], 64, pic.px_rows[c]);
  const int q = ctx->cur;
  int r = grow_block (ctx, ctx->pack_tmp_q[q], ctx->pack_tmp_size_q[q], end);
  *block = (char *) ctx->pack_tmp_q[q];
  return r;
}

// What V210Job, Pack8Job and WideJob have in common, and the picture's planes of levels depth-1 .. 1 for the level loop.
// tiled_width: the columns that tiles of cols x rows cover; tiles: the launch's count so far.
template < class Job > static Job
level_job (const PackPic & pic, char *block, int depth, int bps, int tiled_width, int cols, int rows, int &tiles,
    std::vector < SchroHipIwtPlane > &coarse)
{
  Job j;
  memset (&j, 0, sizeof (j));
  for (int c = 0; c < 3; c++) {
    j.src[c] = pic.src[c];
    j.src_stride[c] = pic.src_stride[c];
    if (depth > 1) {
      // the level-1 view of the coefficient frame {w / 2, h / 2, stride x 2} (schroparams.c:319-352), depth - 1 levels
      SchroHipIwtPlane pl;
      memset (&pl, 0, sizeof (pl));
      pl.src = pic.src[c];
      pl.src_stride = 2 * pic.src_stride[c];
      pl.dst = block + pic.slot[c].at;
      pl.dst_stride = pic.slot[c].stride;
      pl.width = pic.cw (c) >> 1;
      pl.height = pic.ch (c) >> 1;
      coarse.push_back (pl);
      j.ll[c] = pl.dst;
      j.ll_stride[c] = pl.dst_stride;
    } else {
      j.ll[c] = pic.src[c];     // (the frame's LL quadrant)
      j.ll_stride[c] = 2 * pic.src_stride[c];
    }
    // 8-byte loads of the four bands: whole groups of samples per row, 8-byte aligned rows and band origins
    const int nc = pic.cw (c) >> 1, vl = 8 / bps;
    const uintptr_t bits = (uintptr_t) j.ll[c] | (uintptr_t) j.ll_stride[c] | (uintptr_t) pic.src[c] | (uintptr_t) pic.src_stride[c]
        | (uintptr_t) nc * bps;
    if (nc % vl == 0 && nc >= vl && (bits & 7) == 0)
      j.flags |= 1 << c;
  }
  j.w = pic.width;
  j.h = pic.height;
  j.out_w = pic.out_width;
  j.out_h = pic.out_height;
  j.dst = pic.dst;
  j.dst_stride = pic.dst_stride;
  j.tiles_x = div_up (tiled_width, cols);
  j.tile_base = tiles;
  tiles += j.tiles_x * div_up (pic.out_height, rows);
  return j;
}

static int
coarse_levels (SchroHipContext * ctx, const std::vector < SchroHipIwtPlane > &coarse, int depth, int filter, int bps)
{
  return coarse.empty () ? 0 : schro_hip_iiwt_batch (ctx, coarse.data (), (int) coarse.size (), depth - 1, filter, bps);
}

// One launch of a finest-level kernel for its jobs of the call, if it has any: launch (device jobs, their number)
template < class Job, class Launch > static int
finest_level (SchroHipContext * ctx, const std::vector < Job > &jobs, Launch launch)
{
  if (jobs.empty ())
    return 0;
  void *d_jobs = nullptr;
  int r = push_args (ctx, jobs.data (), sizeof (Job) * jobs.size (), &d_jobs);
  if (r)
    return r;
  ProfileScope ps (ctx, SCHRO_HIP_KERNEL_IIWT_FINEST);
  return launch ((const Job *) d_jobs, (int) jobs.size ());
}

// ---- the two passes (the general form) ------------------------------------------------------------------------------
// A picture's three transform planes into the block, and the pack that reads them
static void
two_pass_picture (const PackPic & pic, char *block, int format, std::vector < SchroHipIwtPlane > &planes,
    std::vector < SchroHipPackPlane > &packs)
{
  SchroHipPackPlane pk;
  memset (&pk, 0, sizeof (pk));
  for (int c = 0; c < 3; c++) {
    SchroHipIwtPlane pl;
    memset (&pl, 0, sizeof (pl));
    pl.src = pic.src[c];
    pl.src_stride = pic.src_stride[c];
    pl.dst = block + pic.slot[c].at;
    pl.dst_stride = pic.slot[c].stride;
    pl.width = pic.cw (c);
    pl.height = pic.ch (c);
    planes.push_back (pl);
    pk.src[c] = (const uint8_t *) pl.dst;
    pk.src_stride[c] = pl.dst_stride;
  }
  pk.src_width = pic.out_width; // (the picture inside the transform's padded size: crop, schrovirtframe.c:1823-1853)
  pk.src_height = pic.out_height;
  pk.src_h_shift = pic.h_shift;
  pk.src_v_shift = pic.v_shift;
  pk.dst = pic.dst;
  pk.dst_stride = pic.dst_stride;
  pk.width = pic.out_width;
  pk.height = pic.out_height;
  pk.format = format;
  packs.push_back (pk);
}

// ---- v210 -----------------------------------------------------------------------------------------------------------
extern "C" int
schro_hip_iiwt_pack_v210_batch (SchroHipContext * ctx, const SchroHipIwtPackPicture * pictures, int npictures, int depth, int filter,
    int bytes_per_sample)
{
  const char *who = "iiwt_pack_v210_batch";
  const int bps = bytes_per_sample;
  if (int r = check_call (who, ctx, pictures, npictures, npictures, depth, filter, bps))
    return r;
  (void) hipSetDevice (ctx->device);
  // (experiments: SCHRO_HIP_V210_TWO_PASS=1 sends every picture the Haar kernel does not take to the two passes, for A/B runs)
  const bool level_on = !env_on (SCHRO_ENV ("SCHRO_HIP_V210_TWO_PASS"));
  bool fused = depth == 3 && (filter == 3 || filter == 4) && bps == 4;
  std::vector < HaarPackJob > jobs ((size_t) npictures);
  std::vector < PackPic > pics;
  int tile_base = 0, nlevel = 0;
  for (int p = 0; p < npictures; p++) {
    PackPic pic = common_fields (pictures[p]);
    if (int r = check_geometry (who, p, pic, 16 * ((pic.out_width + 5) / 6)))
      return r;
    // (convert_4xx_422 of s16 / s32 frames is not on the reference's path either: schro_frame_convert finds no match, schroframe.c:869-979)
    SCHRO_HIP_REQUIRE (pic.h_shift == 1 && pic.v_shift == 0, "%s: picture %d: v210 from s16 / s32 frames needs a 4:2:2 frame", who, p);
    for (int c = 0; c < 3; c++) {
      if (int r = check_component (who, p, c, pic, depth, bps))
        return r;
      pic.px_row_bytes[c] = pic.cw (c) * bps;
      pic.px_rows[c] = pic.ch (c);
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
    fused = fused && pic.out_width == pic.width && pic.out_height == pic.height && iiwt_haar3_v210_ok (j);
    pic.level = level_on && level_fits (pic, bps);
    nlevel += pic.level;
    pics.push_back (pic);
  }
  if (fused) {
    int r = finest_level (ctx, jobs, [&](const HaarPackJob * d, int n) { return launch_iiwt_haar3_v210 (ctx->stream, d, n, tile_base, filter); });
    if (!r)
      ctx->v210_routes[SCHRO_HIP_V210_ROUTE_HAAR3] += npictures;
    return r;
  }
  char *block;
  int r = lay_out_block (ctx, pics, depth, bps, &block);
  if (r)
    return r;

  if (nlevel) {
    std::vector < SchroHipIwtPlane > coarse;
    std::vector < V210Job > vj;
    int cols, rows, tiles = 0;
    iiwt_v210_geometry (filter, bps, &cols, &rows);
    for (const PackPic & pic : pics)
      if (pic.level)
        vj.push_back (level_job < V210Job > (pic, block, depth, bps, pic.out_width, cols, rows, tiles, coarse));
    r = coarse_levels (ctx, coarse, depth, filter, bps);
    if (!r)
      r = finest_level (ctx, vj, [&](const V210Job * d, int n) { return launch_iiwt_v210 (ctx->stream, d, n, tiles, filter, bps); });
    if (r)
      return r;
    ctx->v210_routes[SCHRO_HIP_V210_ROUTE_LEVEL] += nlevel;
    if (nlevel == npictures)
      return 0;
  }

  std::vector < SchroHipIwtPlane > planes;
  std::vector < SchroHipPackPlane > packs;
  for (const PackPic & pic : pics)
    if (!pic.level)
      two_pass_picture (pic, block, SCHRO_HIP_FORMAT_v210, planes, packs);
  r = schro_hip_iiwt_batch (ctx, planes.data (), (int) planes.size (), depth, filter, bps);
  if (!r)
    r = schro_hip_pack_v210_batch (ctx, packs.data (), (int) packs.size (), bps);
  if (!r)
    ctx->v210_routes[SCHRO_HIP_V210_ROUTE_TWO_PASS] += (long long) packs.size ();
  return r;
}

extern "C" int
schro_hip_v210_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_V210_ROUTES], int reset)
{
  return read_routes ("v210_routes", ctx, &SchroHipContext::v210_routes, counts, reset);
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

extern "C" int
schro_hip_iiwt_pack_u8_batch (SchroHipContext * ctx, const SchroHipIwtPack8Picture * pictures, int npictures, int depth, int filter,
    int bytes_per_sample)
{
  const char *who = "iiwt_pack_u8_batch";
  const int bps = bytes_per_sample;
  if (int r = check_call (who, ctx, pictures, npictures, 3 * npictures, depth, filter, bps))
    return r;
  (void) hipSetDevice (ctx->device);
  const bool level_on = !env_on (SCHRO_ENV ("SCHRO_HIP_PACK8_TWO_PASS")), level_all = env_on (SCHRO_ENV ("SCHRO_HIP_PACK8_LEVEL"));
  std::vector < PackPic > pics;
  int nlevel = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipIwtPack8Picture & in = pictures[p];
    PackPic pic = common_fields (in);
    SCHRO_HIP_REQUIRE (in.format == SCHRO_HIP_FORMAT_YUYV || in.format == SCHRO_HIP_FORMAT_UYVY || in.format == SCHRO_HIP_FORMAT_AYUV,
        "%s: picture %d: format 0x%x is not YUYV / UYVY / AYUV", who, p, in.format);
    const bool ayuv = in.format == SCHRO_HIP_FORMAT_AYUV;
    if (int r = check_geometry (who, p, pic, ayuv ? 4 * pic.out_width : 4 * (pic.out_width / 2)))
      return r;
    SCHRO_HIP_REQUIRE ((pic.h_shift == 0 || pic.h_shift == 1) && (pic.v_shift == 0 || pic.v_shift == 1) && !(pic.v_shift && !pic.h_shift),
        "%s: picture %d: chroma format not 4:4:4 / 4:2:2 / 4:2:0", who, p);
    const bool has_pred = in.pred[0] != nullptr;
    SCHRO_HIP_REQUIRE ((in.pred[1] != nullptr) == has_pred && (in.pred[2] != nullptr) == has_pred,
        "%s: picture %d: a prediction for some components and not for others", who, p);
    bool fits = bps == 2 && level_on && (level_all || pack8_level_filter (filter, ayuv)) && pic.v_shift == 0 && pic.h_shift == (ayuv ? 0 : 1)
        && level_fits (pic, bps);
    for (int c = 0; c < 3; c++) {
      if (int r = check_component (who, p, c, pic, depth, bps))
        return r;
      // the planar picture of the two passes: u8, the output's size, chroma rounded up
      const int ow = c ? (pic.out_width + pic.h_shift) >> pic.h_shift : pic.out_width;
      const int oh = c ? (pic.out_height + pic.v_shift) >> pic.v_shift : pic.out_height;
      pic.px_row_bytes[c] = ow;
      pic.px_rows[c] = oh;
      SCHRO_HIP_REQUIRE (!has_pred || in.pred_stride[c] >= ow,
          "%s: picture %d component %d: prediction stride %d does not hold %d samples", who, p, c, in.pred_stride[c], ow);
      if (has_pred)
        fits = fits && ((((uintptr_t) in.pred[c] | (uintptr_t) in.pred_stride[c]) & 7) == 0) && in.pred_stride[c] >= ((ow + 7) & ~7)
            && apart (pic.dst, (size_t) pic.dst_stride * pic.out_height, in.pred[c], (size_t) in.pred_stride[c] * oh);
    }
    pic.level = fits;
    nlevel += fits;
    pics.push_back (pic);
  }
  char *block;
  int r = lay_out_block (ctx, pics, depth, bps, &block);
  if (r)
    return r;

  if (nlevel) {
    std::vector < SchroHipIwtPlane > coarse;
    std::vector < Pack8Job > pj[2];     // [0] YUYV / UYVY, [1] AYUV: one launch each
    int tiles[2] = { 0, 0 };
    for (int p = 0; p < npictures; p++) {
      if (!pics[(size_t) p].level)
        continue;
      const SchroHipIwtPack8Picture & in = pictures[p];
      const int ayuv = in.format == SCHRO_HIP_FORMAT_AYUV;
      int cols, rows;
      iiwt_pack8_geometry (filter, ayuv, &cols, &rows);
      Pack8Job j = level_job < Pack8Job > (pics[(size_t) p], block, depth, bps, in.out_width, cols, rows, tiles[ayuv], coarse);
      for (int c = 0; c < 3; c++) {
        j.pred[c] = in.pred[c];
        j.pred_stride[c] = in.pred_stride[c];
      }
      if (in.format == SCHRO_HIP_FORMAT_UYVY)
        j.flags |= 8;
      pj[ayuv].push_back (j);
    }
    r = coarse_levels (ctx, coarse, depth, filter, bps);
    for (int ayuv = 0; ayuv < 2 && !r; ayuv++)
      r = finest_level (ctx, pj[ayuv], [&](const Pack8Job * d, int n) { return launch_iiwt_pack8 (ctx->stream, d, n, tiles[ayuv], filter, ayuv); });
    if (r)
      return r;
    ctx->pack8_routes[SCHRO_HIP_PACK8_ROUTE_LEVEL] += nlevel;
    if (nlevel == npictures)
      return 0;
  }

  // the combine form into planar u8 planes, then the pack
  std::vector < SchroHipIwtPlane > planes;
  std::vector < SchroHipPackPlane > packs;
  for (int p = 0; p < npictures; p++) {
    const PackPic & pic = pics[(size_t) p];
    if (pic.level)
      continue;
    const SchroHipIwtPack8Picture & in = pictures[p];
    two_pass_picture (pic, block, in.format, planes, packs);
    for (int c = 0; c < 3; c++) {
      SchroHipIwtPlane & pl = planes[planes.size () - 3 + (size_t) c];
      pl.combine = in.pred[0] ? 1 : 2;
      pl.pred = in.pred[c];
      pl.pred_stride = in.pred_stride[c];
      pl.out_width = pic.px_row_bytes[c];
      pl.out_height = pic.px_rows[c];
    }
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
  return read_routes ("pack8_routes", ctx, &SchroHipContext::pack8_routes, counts, reset);
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
  const char *who = "iiwt_pack_wide_batch";
  const int bps = bytes_per_sample;
  if (int r = check_call (who, ctx, pictures, npictures, 3 * npictures, depth, filter, bps))
    return r;
  (void) hipSetDevice (ctx->device);
  const bool level_on = !env_on (SCHRO_ENV ("SCHRO_HIP_WIDE_TWO_PASS")), level_all = env_on (SCHRO_ENV ("SCHRO_HIP_WIDE_LEVEL"));
  std::vector < PackPic > pics;
  int nlevel = 0;
  for (int p = 0; p < npictures; p++) {
    const SchroHipIwtPackWidePicture & in = pictures[p];
    PackPic pic = common_fields (in);
    SCHRO_HIP_REQUIRE (is_wide_format (in.format), "%s: picture %d: format 0x%x is not v216 / ARGB / AY64", who, p, in.format);
    const bool v216 = in.format == SCHRO_HIP_FORMAT_v216;
    const int row_bytes = v216 ? 8 * (pic.out_width / 2) : in.format == SCHRO_HIP_FORMAT_ARGB ? 4 * pic.out_width : 8 * pic.out_width;
    if (int r = check_geometry (who, p, pic, row_bytes))
      return r;
    // (no chroma resampling of s16 / s32 frames on the reference's path: as schro_hip_pack_wide_batch)
    SCHRO_HIP_REQUIRE (pic.v_shift == 0 && pic.h_shift == (v216 ? 1 : 0), "%s: picture %d: the source must be %s", who, p,
        v216 ? "4:2:2" : "4:4:4");
    SCHRO_HIP_REQUIRE (in.shift >= 0 && in.shift < 8 * bps, "%s: picture %d: shift %d", who, p, in.shift);
    for (int c = 0; c < 3; c++) {
      if (int r = check_component (who, p, c, pic, depth, bps))
        return r;
      pic.px_row_bytes[c] = pic.cw (c) * bps;
      pic.px_rows[c] = pic.ch (c);
    }
    pic.level = level_on && (level_all || wide_level_combination (in.format, filter, bps)) && row_bytes > 0 && level_fits (pic, bps);
    nlevel += pic.level;
    pics.push_back (pic);
  }
  char *block;
  int r = lay_out_block (ctx, pics, depth, bps, &block);
  if (r)
    return r;

  if (nlevel) {
    std::vector < SchroHipIwtPlane > coarse;
    std::vector < WideJob > wj[2];      // [0] ARGB / AY64, [1] v216: one launch each
    int tiles[2] = { 0, 0 };
    for (int p = 0; p < npictures; p++) {
      if (!pics[(size_t) p].level)
        continue;
      const SchroHipIwtPackWidePicture & in = pictures[p];
      const int v216 = in.format == SCHRO_HIP_FORMAT_v216;
      int cols, rows;
      iiwt_wide_geometry (filter, v216, &cols, &rows);
      // (v216: a tile is `cols` output pairs = luma columns; the luma columns from out_width / 2 on are never lifted)
      WideJob j = level_job < WideJob > (pics[(size_t) p], block, depth, bps, v216 ? in.out_width / 2 : in.out_width, cols, rows,
          tiles[v216], coarse);
      if (in.format == SCHRO_HIP_FORMAT_AY64)
        j.flags |= 8;
      j.shift = in.shift;
      wj[v216].push_back (j);
    }
    r = coarse_levels (ctx, coarse, depth, filter, bps);
    for (int v216 = 0; v216 < 2 && !r; v216++)
      r = finest_level (ctx, wj[v216], [&](const WideJob * d, int n) { return launch_iiwt_wide (ctx->stream, d, n, tiles[v216], filter, bps, v216); });
    if (r)
      return r;
    ctx->wide_routes[SCHRO_HIP_WIDE_ROUTE_LEVEL] += nlevel;
    if (nlevel == npictures)
      return 0;
  }

  // transform into pixel planes, the shift, then the pack
  std::vector < SchroHipIwtPlane > planes;
  std::vector < SchroHipPackPlane > packs;
  std::vector < int >shifts;            // the distinct non-zero shifts of the call
  for (int p = 0; p < npictures; p++) {
    if (pics[(size_t) p].level)
      continue;
    two_pass_picture (pics[(size_t) p], block, pictures[p].format, planes, packs);
    bool seen = pictures[p].shift == 0;
    for (int s : shifts)
      seen = seen || s == pictures[p].shift;
    if (!seen)
      shifts.push_back (pictures[p].shift);
  }
  r = schro_hip_iiwt_batch (ctx, planes.data (), (int) planes.size (), depth, filter, bps);
  for (size_t n = 0; n < shifts.size () && !r; n++) {
    // schro_frame_shift_right on the picture inside each plane (all the packer reads), one launch per distinct shift
    std::vector < SchroHipDcPlane > sp;
    size_t k = 0;
    for (int p = 0; p < npictures; p++) {
      const PackPic & pic = pics[(size_t) p];
      if (pic.level)
        continue;
      for (int c = 0; c < 3; c++, k++) {
        if (pictures[p].shift != shifts[n])
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
  return read_routes ("wide_routes", ctx, &SchroHipContext::wide_routes, counts, reset);
}
