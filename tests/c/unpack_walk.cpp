// unpack_walk.cpp -- the host code of the encoder's way in (plane_unpack.cpp, the packed level 0 of plane_iwt.cpp and the
// frame layer's schro_hipframe_convert_input / schro_hipframe_unpack_iwt_transform) walked under AddressSanitizer +
// UndefinedBehaviorSanitizer: a plain C++ program with its own main, linked with the objects of the library's
// device-free sanitizer build (make -C schroedinger_amd/csrc dry_asan).  Launches are dropped there, so what runs is
// every refusal, the job tables, the routes and the sizing of the queue's blocks -- in a small, large, small order of
// calls on two queues.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "unpack_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

static char *block;
static const size_t kBlock = (size_t) 96 << 20;

static int
row_bytes (int format, int w)
{
  switch (format) {
    case SCHRO_HIP_FORMAT_YUYV:
    case SCHRO_HIP_FORMAT_UYVY: return 4 * (w / 2);
    case SCHRO_HIP_FORMAT_AYUV: return 4 * w;
    case SCHRO_HIP_FORMAT_v210: return 16 * ((w + 5) / 6);
    case SCHRO_HIP_FORMAT_v216: return 8 * (w / 2);
    default: return 8 * w;
  }
}

// a well-formed picture: the source at the block's start, the destination planes behind it
static SchroHipUnpackPicture
good (int format, int sw, int sh, int dst_bpp, int hs, int vs, int w, int h)
{
  SchroHipUnpackPicture p;
  memset (&p, 0, sizeof (p));
  size_t off = 0;
  p.format = format;
  p.src_width = sw;
  p.src_height = sh;
  p.src[0] = block;
  p.src_stride[0] = (row_bytes (format, sw) + 15) / 16 * 16;
  off += (size_t) p.src_stride[0] * sh;
  p.dst_bpp = dst_bpp;
  p.h_shift = hs;
  p.v_shift = vs;
  p.width = w;
  p.height = h;
  for (int k = 0; k < 3; k++) {
    const int cw = k ? (w + hs) >> hs : w, ch = k ? (h + vs) >> vs : h;
    off = (off + 255) / 256 * 256;
    p.dst[k] = block + off;
    p.dst_stride[k] = (cw * dst_bpp + 15) / 16 * 16;
    off += (size_t) p.dst_stride[k] * ch;
  }
  if (off > kBlock) {
    fprintf (stderr, "unpack_walk: the block is too small\n");
    exit (2);
  }
  return p;
}

static SchroHipUnpackPicture
planar (int src_bpp, int shs, int svs, int sw, int sh, int dst_bpp, int hs, int vs, int w, int h)
{
  SchroHipUnpackPicture p = good (SCHRO_HIP_FORMAT_AYUV, sw, sh, dst_bpp, hs, vs, w, h);
  size_t off = ((char *) p.dst[2] - block) + (size_t) p.dst_stride[2] * h;
  p.format = 0;
  p.src_bpp = src_bpp;
  p.src_h_shift = shs;
  p.src_v_shift = svs;
  for (int k = 0; k < 3; k++) {
    off = (off + 255) / 256 * 256;
    p.src[k] = block + off;
    p.src_stride[k] = (sw * src_bpp + 15) / 16 * 16;
    off += (size_t) p.src_stride[k] * sh;
  }
  return p;
}

static int refusals = 0;

static void
refuse (SchroHipContext * ctx, const char *what, SchroHipUnpackPicture p, const char *says)
{
  // a good picture in front: the refusal names picture 1 and nothing of the call is launched
  SchroHipUnpackPicture two[2] = { good (SCHRO_HIP_FORMAT_UYVY, 8, 4, 1, 1, 0, 8, 4), p };
  // (the good picture's planes must not be what the bad one overlaps with)
  const int r = schro_hip_unpack_batch (ctx, two, 2);
  EXPECT (r == SCHRO_HIP_EINVAL, "%s is not refused", what);
  EXPECT (strstr (schro_hip_last_error (), says), "%s: the refusal does not say \"%s\"", what, says);
  refusals++;
}

static SchroHipUnpackIwtPicture
iwt_picture (int format, int hs, int vs, int sw, int sh, int w, int h, int iw, int ih, int bpp, int stride_extra, size_t at)
{
  SchroHipUnpackIwtPicture p;
  memset (&p, 0, sizeof (p));
  size_t off = at;
  p.src = block + off;
  p.src_stride = (row_bytes (format, sw) + 15) / 16 * 16 + stride_extra;
  off += (size_t) p.src_stride * sh;
  p.format = format;
  p.src_width = sw;
  p.src_height = sh;
  p.width = w;
  p.height = h;
  p.h_shift = hs;
  p.v_shift = vs;
  p.iwt_width = iw;
  p.iwt_height = ih;
  for (int k = 0; k < 3; k++) {
    const int cw = k ? (iw + hs) >> hs : iw, ch = k ? (ih + vs) >> vs : ih;
    off = (off + 255) / 256 * 256;
    p.dst[k] = block + off;
    p.dst_stride[k] = (cw * bpp + 63) / 64 * 64;
    off += (size_t) p.dst_stride[k] * ch;
  }
  if (off > kBlock) {
    fprintf (stderr, "unpack_walk: the block is too small\n");
    exit (2);
  }
  return p;
}

int
main ()
{
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "unpack_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
    return 2;
  }
  block = (char *) schro_hip_domain_alloc (ctx, kBlock);
  if (!block) {
    fprintf (stderr, "unpack_walk: no memory: %s\n", schro_hip_last_error ());
    return 2;
  }

  // ---- every accepted source format x destination depth, one call each and all in one ----------------------------
  const int formats[6] = { SCHRO_HIP_FORMAT_YUYV, SCHRO_HIP_FORMAT_UYVY, SCHRO_HIP_FORMAT_AYUV, SCHRO_HIP_FORMAT_v210,
    SCHRO_HIP_FORMAT_v216, SCHRO_HIP_FORMAT_AY64 };
  int accepted = 0;
  for (int f = 0; f < 6; f++)
    for (int bpp = 1; bpp <= 4; bpp *= 2) {
      if (formats[f] == SCHRO_HIP_FORMAT_AY64 && bpp == 1)
        continue;
      const int hs = formats[f] == SCHRO_HIP_FORMAT_AYUV || formats[f] == SCHRO_HIP_FORMAT_AY64 ? 0 : 1;
      SchroHipUnpackPicture p = good (formats[f], 352, 160, bpp, hs, 0, 331, 150);
      EXPECT (schro_hip_unpack_batch (ctx, &p, 1) == 0, "format 0x%x -> %d bytes is refused", formats[f], bpp);
      SchroHipUnpackPicture tiny = good (formats[f], 2, 1, bpp, hs, 0, 2, 1);
      EXPECT (schro_hip_unpack_batch (ctx, &tiny, 1) == 0, "format 0x%x -> %d bytes, 2 x 1, is refused", formats[f], bpp);
      accepted += 2;
    }
  {
    SchroHipUnpackPicture p = planar (1, 1, 1, 150, 62, 2, 1, 1, 160, 64);
    EXPECT (schro_hip_unpack_batch (ctx, &p, 1) == 0, "planar u8 -> s16 is refused");
    SchroHipUnpackPicture q = planar (4, 0, 0, 64, 32, 1, 1, 1, 64, 32);
    EXPECT (schro_hip_unpack_batch (ctx, &q, 1) == 0, "planar s32 4:4:4 -> u8 4:2:0 is refused");
    std::vector < SchroHipUnpackPicture > many (SCHRO_HIP_UNPACK_MAX_PICTURES, good (SCHRO_HIP_FORMAT_v210, 22, 3, 2, 1, 0, 22, 3));
    EXPECT (schro_hip_unpack_batch (ctx, many.data (), (int) many.size ()) == 0, "the largest call is refused");
    many.push_back (many[0]);
    EXPECT (schro_hip_unpack_batch (ctx, many.data (), (int) many.size ()) == SCHRO_HIP_EINVAL, "a call over the limit passes");
    accepted += 3;
  }

  // ---- every refusal ----------------------------------------------------------------------------------------------
  const SchroHipUnpackPicture ayuv = good (SCHRO_HIP_FORMAT_AYUV, 8, 4, 1, 0, 0, 8, 4);
  SchroHipUnpackPicture p;
  p = ayuv, p.format = SCHRO_HIP_FORMAT_ARGB;
  refuse (ctx, "an ARGB source", p, "schrovirtframe.c:693-732");
  refuse (ctx, "AY64 -> u8", good (SCHRO_HIP_FORMAT_AY64, 8, 4, 1, 0, 0, 8, 4), "schroframe.c:908");
  p = good (SCHRO_HIP_FORMAT_YUYV, 8, 4, 1, 1, 0, 7, 4), p.src_width = 7;
  refuse (ctx, "YUYV of odd width", p, "schrovirtframe.c:629");
  p = good (SCHRO_HIP_FORMAT_UYVY, 8, 4, 1, 1, 0, 7, 4), p.src_width = 7;
  refuse (ctx, "UYVY of odd width", p, "schrovirtframe.c:629");
  p = good (SCHRO_HIP_FORMAT_v216, 8, 4, 2, 1, 0, 7, 4), p.src_width = 7;
  refuse (ctx, "v216 of odd width", p, "881");
  refuse (ctx, "a chroma change in s16", good (SCHRO_HIP_FORMAT_AYUV, 8, 4, 2, 1, 0, 8, 4), "schrovirtframe.c:1549-1569");
  refuse (ctx, "a chroma change of v210", good (SCHRO_HIP_FORMAT_v210, 12, 4, 2, 1, 1, 12, 4), "schrovirtframe.c:1549-1569");
  refuse (ctx, "a chroma change of planar s32", planar (4, 0, 0, 8, 4, 4, 1, 0, 8, 4), "schrovirtframe.c:1549-1569");
  refuse (ctx, "wider and shorter", good (SCHRO_HIP_FORMAT_AYUV, 8, 4, 1, 0, 0, 10, 3), "mixes crop and extension");
  refuse (ctx, "narrower and taller", good (SCHRO_HIP_FORMAT_AYUV, 8, 4, 1, 0, 0, 6, 5), "mixes crop and extension");
  p = good (SCHRO_HIP_FORMAT_v210, 12, 4, 2, 1, 0, 12, 4), p.src_stride[0] = 31;
  refuse (ctx, "a source stride below a row", p, "source stride");
  p = planar (2, 1, 0, 8, 4, 2, 1, 0, 8, 4), p.src_stride[1] = 6;
  refuse (ctx, "a planar source stride below a row", p, "source stride");
  p = ayuv, p.dst_stride[0] = 7;
  refuse (ctx, "a destination stride below a row", p, "destination stride");
  p = good (SCHRO_HIP_FORMAT_UYVY, 8, 4, 2, 1, 0, 8, 4), p.dst[1] = (char *) p.dst[1] + 1;
  refuse (ctx, "a misaligned destination", p, "not aligned");
  p = good (SCHRO_HIP_FORMAT_UYVY, 8, 4, 4, 1, 0, 8, 4), p.dst_stride[2] += 2;
  refuse (ctx, "a misaligned destination stride", p, "not aligned");
  p = planar (2, 1, 0, 8, 4, 2, 1, 0, 8, 4), p.src[2] = (const char *) p.src[2] + 1;
  refuse (ctx, "a misaligned planar source", p, "not aligned");
  p = good (SCHRO_HIP_FORMAT_AY64, 8, 4, 4, 0, 0, 8, 4), p.src[0] = (const char *) p.src[0] + 1;
  refuse (ctx, "misaligned AY64 rows", p, "2-byte aligned");
  p = ayuv, p.dst[2] = (char *) block + 3;
  refuse (ctx, "a destination over the source", p, "overlaps a source");
  p = ayuv, p.width = 0;
  refuse (ctx, "no width", p, "must be positive");
  p = ayuv, p.src_height = -1;
  refuse (ctx, "a negative source height", p, "must be positive");
  p = ayuv, p.dst_bpp = 3;
  refuse (ctx, "a destination of 3 bytes", p, "dst_bpp");
  p = planar (3, 0, 0, 8, 4, 1, 0, 0, 8, 4);
  refuse (ctx, "a source of 3 bytes", p, "src_bpp");
  p = ayuv, p.v_shift = 1;
  refuse (ctx, "4:4:0", p, "chroma format");
  p = ayuv, p.format = 0x104;
  refuse (ctx, "an unknown format", p, "no packed format");
  p = ayuv, p.dst[1] = nullptr;
  refuse (ctx, "a NULL destination", p, "NULL");
  p = ayuv, p.src[0] = nullptr;
  refuse (ctx, "a NULL source", p, "NULL");
  EXPECT (schro_hip_unpack_batch (nullptr, &ayuv, 1) == SCHRO_HIP_EINVAL, "no context passes");
  EXPECT (schro_hip_unpack_batch (ctx, nullptr, 1) == SCHRO_HIP_EINVAL, "no pictures pass");
  EXPECT (schro_hip_unpack_batch (ctx, &ayuv, 0) == SCHRO_HIP_EINVAL, "an empty call passes");

  // ---- packed bytes to coefficients: the routes and the block's sizing, small -> large -> small, on two queues -------
  long long routes[SCHRO_HIP_UNPACK_ROUTES];
  EXPECT (schro_hip_unpack_routes (ctx, routes, 1) == 0, "routes");
  int calls = 0;
  for (int queue = 0; queue < 2; queue++) {
    EXPECT (schro_hip_context_select_queue (ctx, queue) == 0, "select queue %d", queue);
    const int sizes[3][2] = { { 64, 32 }, { 1920, 1088 }, { 64, 32 } };
    for (int s = 0; s < 3; s++)
      for (int bpp = 2; bpp <= 4; bpp += 2) {
        const int iw = sizes[s][0], ih = sizes[s][1];
        // a FUSED picture, one of odd stride and one with a chroma change (TWO_PASS: they size the block)
        SchroHipUnpackIwtPicture three[3] = {
          iwt_picture (SCHRO_HIP_FORMAT_v210, 1, 0, iw - 2, ih - 2, iw - 5, ih - 3, iw, ih, bpp, 0, 0),
          iwt_picture (SCHRO_HIP_FORMAT_UYVY, 1, 0, iw, ih, iw - 5, ih - 3, iw, ih, bpp, 1, (size_t) 24 << 20),
          iwt_picture (SCHRO_HIP_FORMAT_AYUV, 1, 1, iw, ih, iw, ih, iw, ih, bpp, 0, (size_t) 48 << 20),
        };
        for (int depth = 1; depth <= 4; depth += 3)
          for (int filter = 0; filter < 7; filter += 3) {
            EXPECT (schro_hip_unpack_iwt_batch (ctx, three, 3, depth, filter, bpp) == 0, "%d x %d, depth %d, filter %d, %d bytes", iw, ih,
                depth, filter, bpp);
            calls++;
          }
      }
  }
  EXPECT (schro_hip_context_select_queue (ctx, 0) == 0, "select queue 0");
  EXPECT (schro_hip_unpack_routes (ctx, routes, 1) == 0, "routes");
  EXPECT (routes[SCHRO_HIP_UNPACK_ROUTE_FUSED] == calls && routes[SCHRO_HIP_UNPACK_ROUTE_TWO_PASS] == 2 * calls,
      "%lld FUSED and %lld TWO_PASS pictures of %d calls", routes[0], routes[1], calls);

  // the call's own refusals: nothing launched, nothing counted
  SchroHipUnpackIwtPicture q = iwt_picture (SCHRO_HIP_FORMAT_UYVY, 1, 0, 64, 32, 64, 32, 64, 32, 2, 0, 0), bad;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &q, 1, 2, 1, 2) == 0, "the good picture is refused");
  bad = q, bad.format = SCHRO_HIP_FORMAT_ARGB;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &bad, 1, 2, 1, 2) == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), "schrovirtframe.c:693"), "ARGB passes");
  bad = q, bad.src_width = 63;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &bad, 1, 2, 1, 2) == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), "schrovirtframe.c:629"), "an odd width passes");
  bad = q, bad.format = SCHRO_HIP_FORMAT_v210, bad.v_shift = 1;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &bad, 1, 2, 1, 2) == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), "schrovirtframe.c:1549"), "a v210 chroma change passes");
  bad = q, bad.iwt_height = 34;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &bad, 1, 2, 1, 2) == SCHRO_HIP_EINVAL, "a size that is no multiple of 4 passes");
  bad = q, bad.iwt_width = 60;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &bad, 1, 2, 1, 2) == SCHRO_HIP_EINVAL, "a transform smaller than the picture passes");
  bad = q, bad.dst[1] = (char *) q.src + 8;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &bad, 1, 2, 1, 2) == SCHRO_HIP_EINVAL, "coefficients over the source pass");
  bad = q, bad.src_stride = 100;
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &bad, 1, 2, 1, 2) == SCHRO_HIP_EINVAL, "a short source stride passes");
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &q, 1, 0, 1, 2) == SCHRO_HIP_EINVAL, "depth 0 passes");
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &q, 1, 2, 7, 2) == SCHRO_HIP_EINVAL, "filter 7 passes");
  EXPECT (schro_hip_unpack_iwt_batch (ctx, &q, 1, 2, 1, 1) == SCHRO_HIP_EINVAL, "u8 coefficients pass");
  EXPECT (schro_hip_unpack_routes (ctx, routes, 1) == 0 && routes[0] == 1 && routes[1] == 0, "a refused call is counted");
  EXPECT (schro_hip_unpack_routes (nullptr, routes, 0) == SCHRO_HIP_EINVAL, "routes without a context pass");

  // the frame layer without frames
  EXPECT (schro_hipframe_convert_input (nullptr, nullptr) == SCHRO_HIP_EINVAL, "convert_input without frames passes");
  EXPECT (schro_hipframe_unpack_iwt_transform (nullptr, nullptr, nullptr, 0, 0) == SCHRO_HIP_EINVAL, "unpack_iwt_transform without frames passes");

  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  schro_hip_domain_free (ctx, block);
  schro_hip_context_free (ctx);
  printf ("unpack_walk: %d accepted, %d refusals, %d transform calls, %s\n", accepted, refusals, calls, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
