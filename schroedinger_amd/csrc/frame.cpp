// frame.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), third part: the frame layer -- the reference's
// own objects (SchroFrame / SchroParams / SchroMotion-shaped) and the stage calls a patched schrodecoder.c makes
// (schro_frame_inverse_iwt_transform_hip, schro_upsampled_hipframe_upsample, schro_motion_render_hip,
// schro_hipframe_convert ...), built on the plane layer (plane_*.cpp, iiwt_pack.cpp).

#include "schro_hip_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>

using namespace schro;

static SchroHipContext *
frame_ctx (const SchroHipFrame * f)
{
  if (!f || !f->domain || !(f->domain->flags & SCHRO_MEMORY_DOMAIN_HIP))
    return nullptr;
  return f->domain->ctx;
}

static int
format_bpp (int format)
{
  switch (SCHRO_HIP_FORMAT_DEPTH (format)) {
    case SCHRO_HIP_FORMAT_DEPTH_U8:
      return 1;
    case SCHRO_HIP_FORMAT_DEPTH_S16:
      return 2;
    case SCHRO_HIP_FORMAT_DEPTH_S32:
      return 4;
  }
  return 0;
}

// ---- the pieces the transform-data calls stand on: each blind to its caller ----------------------

// a refusal (or failure) of a piece is the call's
#define SCHRO_HIP_TRY(call) do { if (const int r_ = (call)) return r_; } while (0)

// The transform size of component k (SchroHipParams and SchroHipLowDelayParams name the four members alike).
struct IwtSize {
  int w, h;
};
template < typename Params > static IwtSize
iwt_size (const Params * params, int k)
{
  if (k)
    return { params->iwt_chroma_width, params->iwt_chroma_height };
  return { params->iwt_luma_width, params->iwt_luma_height };
}

// a component holds that size; bpp != 0: the size is one, and the stride holds a row of it
static bool
holds (const SchroHipFrameData & c, IwtSize s, int bpp)
{
  return s.w <= c.width && s.h <= c.height && (!bpp || (s.w > 0 && s.h > 0 && (long long) c.stride >= (long long) s.w * bpp));
}

// ... said in the two wordings the calls have: bpp 0 the pixel path's and the slice calls', else the noarith calls'
static int
require_holds (const char *who, int k, const SchroHipFrameData & c, IwtSize s, int bpp)
{
  if (bpp)
    SCHRO_HIP_REQUIRE (holds (c, s, bpp), "%s: component %d (%d x %d, stride %d) does not hold the %d x %d transform", who, k, c.width,
        c.height, c.stride, s.w, s.h);
  else
    SCHRO_HIP_REQUIRE (holds (c, s, 0), "%s: component %d smaller than the iwt size", who, k);
  return 0;
}

// The members the three fused-picture structs (include/schro_hip.h) share, and the refusals their calls share.  `v210`:
// that call's refusals as they have been since r05 -- one text for "not shifted" and "smaller", of the components the luma
// alone, the packed frame's size left to the plane layer; the others refuse each on its own.  `also (k)`: what a call
// adds to component k, a refusal of its own included, in its place behind that component's.
template < typename Picture, typename PerComponent > static int
fill_fused_picture (Picture & pic, const SchroHipFrame * packed, const SchroHipFrame * transform_frame, const SchroHipParams * params,
    bool v210, PerComponent also)
{
  const char *who = "inverse_iwt_transform_convert";
  const IwtSize luma = iwt_size (params, 0), chroma = iwt_size (params, 1);
  memset (&pic, 0, sizeof (pic));
  pic.width = luma.w;
  pic.height = luma.h;
  pic.h_shift = SCHRO_HIP_FORMAT_H_SHIFT (transform_frame->format);
  pic.v_shift = SCHRO_HIP_FORMAT_V_SHIFT (transform_frame->format);
  const bool shifted = (chroma.w << pic.h_shift) == luma.w && (chroma.h << pic.v_shift) == luma.h;
  if (v210) {
    SCHRO_HIP_REQUIRE (holds (transform_frame->components[0], luma, 0) && shifted,
        "%s: the frame is smaller than params' transform size (or the chroma size is not the luma size shifted)", who);
  } else {
    SCHRO_HIP_REQUIRE (shifted, "%s: params' chroma transform size is not the luma size shifted by the frame's chroma format", who);
    SCHRO_HIP_REQUIRE (packed->width <= luma.w && packed->height <= luma.h, "%s: the packed frame is larger than the transform", who);
  }
  pic.dst = (uint8_t *) packed->components[0].data;
  pic.dst_stride = packed->components[0].stride;
  pic.out_width = packed->width;
  pic.out_height = packed->height;
  for (int k = 0; k < 3; k++) {
    SCHRO_HIP_TRY (v210 ? 0 : require_holds (who, k, transform_frame->components[k], iwt_size (params, k), 0));
    pic.src[k] = transform_frame->components[k].data;
    pic.src_stride[k] = transform_frame->components[k].stride;
    SCHRO_HIP_TRY (also (k));
  }
  return 0;
}

// One block of the domain for a call that copies up, runs its batch, copies down and waits for it: three parts one behind
// the other, the second and third at multiples of `align` -- the result in front (kResultFront or kNoarithDecodeFront
// bytes), then the field, then the bytes, for the calls that have a result.  The calls make their own copies; finish ()
// waits (unless wait () already has, for the calls that fetch the bytes once the result has told how many), frees, and
// gives r or else what the wait said.
constexpr size_t kResultFront = 256, kNoarithDecodeFront = 512;
static_assert (sizeof (SchroHipNoarithResult) <= kResultFront && sizeof (SchroHipMotionEncodeResult) <= kResultFront
    && sizeof (SchroHipMotionDecodeResult) <= kResultFront && sizeof (SchroHipMotionArithDecodeResult) <= kResultFront, "the result sits in front of the field and the bytes");
static_assert (sizeof (SchroHipNoarithDecodeResult) <= kNoarithDecodeFront, "the result sits in front of the bytes");

enum { kFront, kField, kBytes };        // (the parts of a call with a result)
struct SyncBlock {
  SchroHipContext *ctx;
  const size_t at[3];
  char *d;                      // NULL: no memory (the allocation has said so)
  int rs = 0;
  bool waited = false;
    SyncBlock (SchroHipContext * c, size_t first, size_t second, size_t third, size_t align = 256):ctx (c),
      at { 0, round_up (first, align), round_up (first, align) + round_up (second, align) },
      d ((char *) schro_hip_domain_alloc (c, at[2] + (third ? third : 1)))
  {
  }
  ~SyncBlock ()
  {
    if (d)
      schro_hip_domain_free (ctx, d);
  }
  char *part (int i) const
  {
    return d + at[i];
  }
  int wait ()
  {
    waited = true;
    return rs = schro_hip_synchronize (ctx);
  }
  int finish (int r)
  {
    if (!waited)
      wait ();                  // the host buffers are filled, d is free again
    schro_hip_domain_free (ctx, d);
    d = nullptr;
    return r ? r : rs;
  }
};

// the LL bands of an intra picture, for schro_hip_dc_predict_batch
static void
ll_planes (SchroHipDcPlane ll[3], const SchroHipFrame * transform_frame, const SchroHipParams * params)
{
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & c = transform_frame->components[k];
    const IwtSize s = iwt_size (params, k);
    ll[k].data = c.data;
    ll[k].stride = c.stride << params->transform_depth; // schro_subband_get_frame_data, schroparams.c:319-352
    ll[k].width = s.w >> params->transform_depth;
    ll[k].height = s.h >> params->transform_depth;
  }
}

// the codeblock records of component k, laid out for its stride
static int
layout_records (const char *who, int k, IwtSize s, const SchroHipParams * params, int stride, int bpp, std::vector < SchroHipCodeblock > &recs)
{
  const int depth = params->transform_depth;
  const int n = schro_hip_codeblock_layout (s.w, s.h, depth, params->horiz_codeblocks, params->vert_codeblocks, stride, bpp, nullptr, 0);
  if (n <= 0)
    return n < 0 ? n : set_error (SCHRO_HIP_EINVAL, "%s: component %d has no codeblocks", who, k);
  recs.resize (n);
  (void) schro_hip_codeblock_layout (s.w, s.h, depth, params->horiz_codeblocks, params->vert_codeblocks, stride, bpp, recs.data (), n);
  return 0;
}

// ... and a call's quant indices in them
static int
set_quant_indices (const char *who, int k, std::vector < SchroHipCodeblock > &recs, const int *quant_indices)
{
  for (size_t c = 0; c < recs.size (); c++) {
    SCHRO_HIP_REQUIRE (quant_indices[c] >= 0 && quant_indices[c] <= 60, "%s: component %d, codeblock %d: quant index %d", who, k, (int) c,
        quant_indices[c]);
    recs[c].quant_index = (unsigned char) quant_indices[c];
  }
  return 0;
}

// the header fields of the two noarith picture structs
template < typename Picture > static void
fill_noarith_header (Picture & pic, const SchroHipParams * params)
{
  memset (&pic, 0, sizeof (pic));
  pic.transform_depth = params->transform_depth;
  pic.codeblock_mode_index = params->codeblock_mode_index;
  for (int l = 0; l <= params->transform_depth; l++) {
    pic.horiz_codeblocks[l] = params->horiz_codeblocks[l];
    pic.vert_codeblocks[l] = params->vert_codeblocks[l];
  }
}

// what the context's tables of a picture geometry (FrameQuantTable, FrameHistTable) were laid out for
static std::vector < int >
table_key (const SchroHipFrame * iwt_frame, const SchroHipParams * params, int bpp)
{
  return { bpp, params->transform_depth, params->iwt_luma_width, params->iwt_luma_height, params->iwt_chroma_width, params->iwt_chroma_height,
    iwt_frame->components[0].stride, iwt_frame->components[1].stride, iwt_frame->components[2].stride };
}

// dest and src over the components' common size (schro_frame_add, _subtract, the s16 -> u8 convert)
static void
common_planes (SchroHipConvertPlane planes[3], const SchroHipFrame * dest, const SchroHipFrame * src)
{
  for (int k = 0; k < 3; k++) {
    planes[k].src = src->components[k].data;
    planes[k].src_stride = src->components[k].stride;
    planes[k].dst = (uint8_t *) dest->components[k].data;
    planes[k].dst_stride = dest->components[k].stride;
    planes[k].width = std::min (dest->components[k].width, src->components[k].width);
    planes[k].height = std::min (dest->components[k].height, src->components[k].height);
  }
}

extern "C" {

// ---- frame layer -----------------------------------------------------------------

// How a stage call ends.  The reference's scheduler expects a stage complete when its function returns
// (schroasync-pthread.c:320-328): the default -- the selected queue is waited for (that queue only: r03
// drained all four).  A host that pipelines pictures itself turns that off
// (schro_hip_context_set_stage_completion (ctx, 0)): the same calls then only enqueue on the selected
// queue, and marks / schro_hip_queue_synchronize order and end them.
static int
stage_done (SchroHipContext * ctx, int r)
{
  if (r || !ctx->stage_complete)
    return r;
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  r = dc_gave_up (ctx);
  return r ? r : pred_overflow_poll (ctx);
}

int
schro_hip_context_set_stage_completion (SchroHipContext * ctx, int complete_on_return)
{
  SCHRO_HIP_REQUIRE (ctx, "set_stage_completion: no context");
  ctx->stage_complete = complete_on_return != 0;
  return 0;
}

SchroHipFrame *
schro_hip_frame_new_and_alloc (SchroHipContext * ctx, int format, int width, int height,
    int upsampled)
{
  if (ctx && width > 0 && height > 0 && !upsampled && (format == SCHRO_HIP_FORMAT_YUYV
          || format == SCHRO_HIP_FORMAT_UYVY || format == SCHRO_HIP_FORMAT_AYUV || format == SCHRO_HIP_FORMAT_v210
          || is_wide_format (format))) {
    // packed output frame: one component (schroframe.c:81-99)
    SchroHipFrame *f = (SchroHipFrame *) calloc (1, sizeof (SchroHipFrame));
    f->refcount = 1;
    f->domain = ctx->domain;
    f->format = format;
    f->width = width;
    f->height = height;
    SchroHipFrameData *c = &f->components[0];
    c->format = format;
    c->width = width;
    c->height = height;
    const size_t row = format == SCHRO_HIP_FORMAT_AYUV || format == SCHRO_HIP_FORMAT_ARGB ? (size_t) width * 4
        : format == SCHRO_HIP_FORMAT_AY64 ? (size_t) width * 8
        : format == SCHRO_HIP_FORMAT_v216 ? (size_t) ((width + 1) & ~1) * 4
        : format == SCHRO_HIP_FORMAT_v210 ? (size_t) 16 * div_up (width, 6) : (size_t) ((width + 1) & ~1) * 2;
    c->stride = (int) round_up (row, 64);
    c->length = c->stride * height;
    c->data = schro_hip_domain_alloc (ctx, round_up ((size_t) c->length, 256));
    if (!c->data) {
      free (f);
      return nullptr;
    }
    f->regions[0] = c->data;
    return f;
  }
  int bpp = format_bpp (format);
  if (!ctx || !bpp || width <= 0 || height <= 0 || (format & 0x100) || (upsampled && bpp != 1)) {
    set_error (SCHRO_HIP_EINVAL, "frame_new_and_alloc: bad arguments");
    return nullptr;
  }
  SchroHipFrame *f = (SchroHipFrame *) calloc (1, sizeof (SchroHipFrame));
  f->refcount = 1;
  f->domain = ctx->domain;
  f->format = format;
  f->width = width;
  f->height = height;
  int h_shift = SCHRO_HIP_FORMAT_H_SHIFT (format), v_shift = SCHRO_HIP_FORMAT_V_SHIFT (format);
  // r04: the chroma of a horizontally subsampled upsampled frame is ONE pair image (is_upsampled == 2):
  // components[1] holds it, components[2] points at the same bytes (length 0: nothing of its own)
  const bool pair = upsampled && h_shift == 1;
  f->is_upsampled = pair ? 2 : upsampled ? 1 : 0;
  // chroma size rounds up, schroframe.c:95-96
  int cw = (width + (1 << h_shift) - 1) >> h_shift, ch = (height + (1 << v_shift) - 1) >> v_shift;
  size_t total = 0;
  for (int k = 0; k < 3; k++) {
    SchroHipFrameData *c = &f->components[k];
    c->format = format;
    c->width = k ? cw : width;
    c->height = k ? ch : height;
    c->h_shift = k ? h_shift : 0;
    c->v_shift = k ? v_shift : 0;
    c->stride = (int) round_up ((size_t) c->width * bpp, 64);
    c->length = c->stride * c->height;
    if (upsampled) {            // the four half-pel planes, tiled (include/schro_hip.h): stride = bytes per band of 4 rows
      int st = 0;
      c->length = (int) (pair && k ? schro_hip_upsampled_pair_bytes (c->width, c->height, &st)
          : schro_hip_upsampled_bytes (c->width, c->height, &st));
      c->stride = st;
      if (pair && k == 2)
        c->length = 0;
    }
    total += round_up ((size_t) c->length, 256);
  }
  void *base = schro_hip_domain_alloc (ctx, total);
  if (!base) {
    free (f);
    return nullptr;
  }
  f->regions[0] = base;
  size_t off = 0;
  for (int k = 0; k < 3; k++) {
    f->components[k].data = (char *) base + off;
    off += round_up ((size_t) f->components[k].length, 256);
  }
  if (pair)
    f->components[2].data = f->components[1].data;
  return f;
}

SchroHipFrame *
schro_hip_frame_ref (SchroHipFrame * frame)
{
  if (frame)
    frame->refcount++;
  return frame;
}

void
schro_hip_frame_unref (SchroHipFrame * frame)
{
  if (!frame)
    return;
  if (--frame->refcount > 0)
    return;
  if (frame_ctx (frame) && frame->regions[0])
    schro_hip_domain_free (frame_ctx (frame), frame->regions[0]);
  free (frame);
}

// all components of a frame, host <-> device or device -> device, on the selected queue; no wait
static int
copy_frame_async (SchroHipContext * ctx, SchroHipFrame * dest, const SchroHipFrame * src, hipMemcpyKind kind)
{
  if ((src->format & 0x100) || (dest->format & 0x100)) {
    SCHRO_HIP_REQUIRE (src->format == dest->format, "frame copy: packed format mismatch");
    const SchroHipFrameData *s = &src->components[0];
    SchroHipFrameData *d = &dest->components[0];
    int w = std::min (s->width, d->width), h = std::min (s->height, d->height);
    const int f = src->format;
    size_t row = f == SCHRO_HIP_FORMAT_AYUV || f == SCHRO_HIP_FORMAT_ARGB ? (size_t) w * 4
        : f == SCHRO_HIP_FORMAT_AY64 ? (size_t) w * 8 : f == SCHRO_HIP_FORMAT_v216 ? (size_t) (w / 2) * 8
        : f == SCHRO_HIP_FORMAT_v210 ? (size_t) 16 * div_up (w, 6) : (size_t) (w / 2) * 4;
    if (row && h > 0)
      return copy_2d_async (ctx, d->data, d->stride, s->data, s->stride, (int) row, h, kind);
    return 0;
  }
  int bpp = format_bpp (src->format);
  SCHRO_HIP_REQUIRE (bpp && format_bpp (dest->format) == bpp, "frame copy: depth mismatch");
  // (r04) Frames as the domains hand them out -- the components one behind the other in ONE block, the same sizes and
  // strides on both sides -- cross as one copy: three copies per 2160p frame cost the pipelined frame layer 0.05 ms per
  // picture.  (The row padding of such a frame belongs to it: copying it too is harmless.)
  {
    bool one = true;
    size_t total = 0;
    for (int k = 0; k < 3 && one; k++) {
      const SchroHipFrameData *s = &src->components[k];
      const SchroHipFrameData *d = &dest->components[k];
      one = s->data && d->data && s->width == d->width && s->height == d->height && s->width > 0 && s->height > 0
          && s->stride == d->stride && s->stride >= s->width * bpp && s->length == d->length
          && (size_t) s->length == (size_t) s->stride * s->height
          && (const uint8_t *) s->data == (const uint8_t *) src->components[0].data + total
          && (const uint8_t *) d->data == (const uint8_t *) dest->components[0].data + total;
      total += (size_t) s->length;
    }
    if (one && total < ((size_t) 1 << 31))
      return copy_2d_async (ctx, dest->components[0].data, (int) total, src->components[0].data, (int) total, (int) total, 1, kind);
  }
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData *s = &src->components[k];
    SchroHipFrameData *d = &dest->components[k];
    int w = std::min (s->width, d->width), h = std::min (s->height, d->height);
    if (w <= 0 || h <= 0)
      continue;
    int r = copy_2d_async (ctx, d->data, d->stride, s->data, s->stride, w * bpp, h, kind);
    if (r)
      return r;
  }
  return 0;
}

static int
copy_frame (SchroHipContext * ctx, SchroHipFrame * dest, const SchroHipFrame * src, hipMemcpyKind kind)
{
  int r = copy_frame_async (ctx, dest, src, kind);
  if (r)
    return r;
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

int
schro_frame_to_hip (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (dest) && !frame_ctx (src),
      "frame_to_hip: dest must be a device frame and src a host frame");
  return copy_frame (frame_ctx (dest), dest, src, hipMemcpyHostToDevice);
}

int
schro_hipframe_to_cpu (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (src) && !frame_ctx (dest),
      "hipframe_to_cpu: src must be a device frame and dest a host frame");
  return copy_frame (frame_ctx (src), dest, src, hipMemcpyDeviceToHost);
}

// r03 -- the asynchronous twins (TODO-CUDA:5-7 "make gpu stuff completely asynchronous"; the
// synchronous pattern they replace: schrogpuframe.c:480-609): enqueued on the context's selected
// queue -- SCHRO_HIP_QUEUE_H2D / _D2H by convention -- and not waited for.  The host frame should live in
// pinned memory (schro_memory_domain_new_hip_host): then picture k's copies run on the DMA engines
// beside picture k - 1's kernels; order them against the stages with marks and end with
// schro_hip_queue_synchronize.
int
schro_frame_to_hip_async (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (dest) && !frame_ctx (src),
      "frame_to_hip_async: dest must be a device frame and src a host frame");
  (void) hipSetDevice (frame_ctx (dest)->device);
  return copy_frame_async (frame_ctx (dest), dest, src, hipMemcpyHostToDevice);
}

int
schro_hipframe_to_cpu_async (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (src) && !frame_ctx (dest),
      "hipframe_to_cpu_async: src must be a device frame and dest a host frame");
  (void) hipSetDevice (frame_ctx (src)->device);
  return copy_frame_async (frame_ctx (src), dest, src, hipMemcpyDeviceToHost);
}

}                               // extern "C"

namespace schro {
// A copy of a device frame on another context's device (the scheduler moves a reference across two
// chains with it): same format, size and layout -- plain or upsampled --, one
// hipMemcpyPeerAsync per component on the destination context's host-to-device COPY queue, behind
// `wait_for` (the owner's event: all the work that writes `src`); `done` is recorded behind the copies
// and the destination's kernel queues wait for it.  Nothing is waited for on the host (r04).  (ROCm 7.2 holds the
// caller of an asynchronous copy from / to pinned HOST memory behind an unfired event; this PEER copy
// measured 22 us in the call with 7 ms of producer work outstanding -- two contexts on one device,
// profiles/r05_peer_copy_hip_trace.txt; between two real devices unmeasured.)
SchroHipFrame *
frame_copy_to_async (SchroHipContext * dst_ctx, SchroHipFrame * src, hipEvent_t wait_for, hipEvent_t done)
{
  SchroHipContext *src_ctx = frame_ctx (src);
  if (!dst_ctx || !src_ctx) {
    set_error (SCHRO_HIP_EINVAL, "frame_copy_to: needs a destination context and a device frame");
    return nullptr;
  }
  SchroHipFrame *dst = schro_hip_frame_new_and_alloc (dst_ctx, src->format, src->width, src->height, src->is_upsampled ? 1 : 0);
  if (!dst)
    return nullptr;
  (void) hipSetDevice (dst_ctx->device);
  hipStream_t q = dst_ctx->streams[SCHRO_HIP_QUEUE_H2D];
  const int ncomp = (src->format & 0x100) ? 1 : 3;
  bool ok = dst->is_upsampled == src->is_upsampled && (!wait_for || hipStreamWaitEvent (q, wait_for, 0) == hipSuccess);
  for (int k = 0; ok && k < ncomp; k++) {
    const SchroHipFrameData *s = &src->components[k];
    SchroHipFrameData *d = &dst->components[k];
    ok = d->length == s->length && d->stride == s->stride
        && (s->length == 0        // (the V component of a pair image: components[1] carries it)
        || hipMemcpyPeerAsync (d->data, dst_ctx->device, s->data, src_ctx->device, (size_t) s->length, q) == hipSuccess);
  }
  if (ok && done) {
    ok = hipEventRecord (done, q) == hipSuccess;
    for (int k = 0; ok && k < 2; k++)
      ok = hipStreamWaitEvent (dst_ctx->streams[k], done, 0) == hipSuccess;
  }
  if (!ok) {
    set_error (SCHRO_HIP_EDEVICE, "frame_copy_to: peer copy device %d -> %d failed", src_ctx->device, dst_ctx->device);
    (void) hipStreamSynchronize (q);
    schro_hip_frame_unref (dst);
    return nullptr;
  }
  dst->upsample_done = src->upsample_done;
  return dst;
}
}                               // namespace schro

extern "C" {

// the synchronous form: complete on return
SchroHipFrame *
schro_hip_frame_copy_to (SchroHipContext * dst_ctx, SchroHipFrame * src)
{
  SchroHipFrame *dst = schro::frame_copy_to_async (dst_ctx, src, nullptr, nullptr);
  if (dst && hipStreamSynchronize (dst_ctx->streams[SCHRO_HIP_QUEUE_H2D]) != hipSuccess) {
    set_error (SCHRO_HIP_EDEVICE, "frame_copy_to: the copy queue of device %d failed", dst_ctx->device);
    schro_hip_frame_unref (dst);
    return nullptr;
  }
  return dst;
}

// schro_gpuframe_iwt_transform (schrogpuframe.h:13-31): the forward transform of a device frame in place.  The level
// kernels are out of place, so the plane layer copies the source planes into the queue's scratch first.
int
schro_hipframe_iwt_transform (SchroHipContext * ctx, SchroHipFrame * frame, const SchroHipParams * params)
{
  SCHRO_HIP_REQUIRE (ctx && frame && params && frame_ctx (frame) == ctx, "hipframe_iwt_transform: the frame must be in the context's domain");
  const int bpp = format_bpp (frame->format);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "hipframe_iwt_transform: the frame must be s16 or s32");
  SchroHipIwtFwdPlane planes[3];
  memset (planes, 0, sizeof (planes));
  for (int k = 0; k < 3; k++) {
    planes[k].src = planes[k].dst = frame->components[k].data;
    planes[k].src_stride = planes[k].dst_stride = frame->components[k].stride;
    const IwtSize s = iwt_size (params, k);
    planes[k].width = s.w;
    planes[k].height = s.h;
    SCHRO_HIP_TRY (require_holds ("hipframe_iwt_transform", k, frame->components[k], s, 0));
  }
  return stage_done (ctx, iwt_batch_run (ctx, planes, 3, params->transform_depth, params->wavelet_filter_index, bpp, true));
}

// frame: the residual frame (s16 / s32, combine 0) or the u8 picture (combine 1: + prediction, 2: + 128)
static int
inverse_iwt_transform (SchroHipFrame * frame, SchroHipFrame * transform_frame, SchroHipParams * params, int combine,
    SchroHipFrame * prediction)
{
  SCHRO_HIP_REQUIRE (frame && transform_frame && params && frame_ctx (frame),
      "inverse_iwt_transform: bad arguments");
  SchroHipContext *ctx = frame_ctx (frame);
  int bpp = format_bpp (transform_frame->format);
  SCHRO_HIP_REQUIRE ((bpp == 2 || bpp == 4) && (combine ? format_bpp (frame->format) == 1 : format_bpp (frame->format) == bpp),
      "inverse_iwt_transform: the transform frame must be s16 or s32, the destination the same (the u8 picture in the combine form)");
  SCHRO_HIP_REQUIRE (combine != 1 || (prediction && prediction->domain == frame->domain && format_bpp (prediction->format) == 1),
      "inverse_iwt_transform: the combine form needs the u8 prediction frame of schro_motion_render_hip (add = FALSE) in the same domain");

  // host coefficients are staged on the device first (the H2D step of
  // schro_frame_inverse_iwt_transform_cuda, schrogpuframe.c:584-599)
  std::unique_ptr < SchroHipFrame, void (*)(SchroHipFrame *) > staged (nullptr, schro_hip_frame_unref);
  SchroHipFrame *src = transform_frame;
  SCHRO_HIP_REQUIRE (ctx->stage_complete || frame_ctx (transform_frame),
      "inverse_iwt_transform: with stage completion off the transform frame must be on the device "
      "(schro_frame_to_hip_async on the copy queue)");
  if (!frame_ctx (transform_frame)) {
    staged.reset (schro_hip_frame_new_and_alloc (ctx, transform_frame->format, transform_frame->width, transform_frame->height, 0));
    if (!staged)
      return SCHRO_HIP_ENOMEM;
    SCHRO_HIP_TRY (schro_frame_to_hip (staged.get (), transform_frame));
    src = staged.get ();
  }
  const char *who = "inverse_iwt_transform";
  SchroHipIwtPlane planes[3];
  memset (planes, 0, sizeof (planes));
  for (int k = 0; k < 3; k++) {
    const IwtSize s = iwt_size (params, k);
    planes[k].src = src->components[k].data;
    planes[k].src_stride = src->components[k].stride;
    planes[k].dst = frame->components[k].data;
    planes[k].dst_stride = frame->components[k].stride;
    planes[k].width = s.w;
    planes[k].height = s.h;
    SCHRO_HIP_TRY (require_holds (who, k, src->components[k], s, 0));
    if (combine) {
      // the picture inside the transform's size (schrodecoder.c:1788-1790 converts with a crop; the render adds
      // over motion->width x height)
      planes[k].combine = combine;
      planes[k].out_width = std::min (frame->components[k].width, s.w);
      planes[k].out_height = std::min (frame->components[k].height, s.h);
      if (combine == 1) {
        planes[k].pred = (const uint8_t *) prediction->components[k].data;
        planes[k].pred_stride = prediction->components[k].stride;
        SCHRO_HIP_TRY (require_holds (who, k, prediction->components[k], { planes[k].out_width, planes[k].out_height }, 0));
      }
    } else {
      SCHRO_HIP_TRY (require_holds (who, k, frame->components[k], s, 0));
    }
  }
  // (staged is released when the call returns: stage_done has waited for the queue -- it is a host frame's, above)
  return stage_done (ctx, schro_hip_iiwt_batch (ctx, planes, 3, params->transform_depth, params->wavelet_filter_index, bpp));
}

int
schro_frame_inverse_iwt_transform_hip (SchroHipFrame * frame,
    SchroHipFrame * transform_frame, SchroHipParams * params)
{
  return inverse_iwt_transform (frame, transform_frame, params, 0, nullptr);
}

// r04 -- x_wavelet_transform and the add of x_combine in one call (the structure of the reference's GPU paths:
// x_render_motion renders the prediction into mc_tmp_frame, x_combine adds, schrodecoder.c:1742-1760, :1908-1921):
// output = sat_u8 (inverse transform (transform_frame) + prediction), or + 128 where prediction is NULL (a picture
// without references, :1788-1790).  The residual picture never exists in memory.
int
schro_frame_inverse_iwt_transform_combine_hip (SchroHipFrame * output_frame, SchroHipFrame * transform_frame,
    SchroHipParams * params, SchroHipFrame * prediction)
{
  return inverse_iwt_transform (output_frame, transform_frame, params, prediction ? 1 : 2, prediction);
}

// r05 -- x_wavelet_transform and x_combine's schro_frame_convert into a v210 output picture in one call, for a picture
// without references (schrodecoder.c:1855-1886 + :2011-2052; the > 8-bit shift of :2013-2019 is 0 when the stream's depth
// is the output's): `packed` is a DEVICE frame of format v210, the transform frame a device s16 / s32 4:2:2 frame.  The
// pixel frame (picture->frame) is not written where the fused kernel applies (schro_hip_iiwt_pack_v210_batch).
// ... and into a YUYV, UYVY or AYUV output picture, with the prediction of an inter picture that is not a reference
// (prediction != NULL: the u8 frame schro_motion_render_hip (add = FALSE) wrote; x_combine's add, :1908-1921) or + 128:
// schro_hip_iiwt_pack_u8_batch.  The planar picture is not written where its fused kernel applies.
static int
inverse_iwt_transform_pack8 (SchroHipFrame * packed, SchroHipFrame * transform_frame, SchroHipParams * params, SchroHipFrame * prediction, int bpp)
{
  SchroHipContext *ctx = frame_ctx (packed);
  SCHRO_HIP_REQUIRE (!prediction || (prediction->domain == packed->domain && format_bpp (prediction->format) == 1),
      "inverse_iwt_transform_combine_convert: the prediction must be the u8 frame of schro_motion_render_hip (add = FALSE) in the same domain");
  SchroHipIwtPack8Picture pic;
  SCHRO_HIP_TRY (fill_fused_picture (pic, packed, transform_frame, params, false,[&](int k) {
        if (!prediction)
          return 0;
        const int ow = k ? (pic.out_width + pic.h_shift) >> pic.h_shift : pic.out_width;
        const int oh = k ? (pic.out_height + pic.v_shift) >> pic.v_shift : pic.out_height;
        SCHRO_HIP_REQUIRE (prediction->components[k].width >= ow && prediction->components[k].height >= oh,
            "inverse_iwt_transform_combine_convert: component %d of the prediction is smaller than the picture", k);
        pic.pred[k] = (const uint8_t *) prediction->components[k].data;
        pic.pred_stride[k] = prediction->components[k].stride;
        return 0;
      }));
  pic.format = packed->format;
  return stage_done (ctx, schro_hip_iiwt_pack_u8_batch (ctx, &pic, 1, params->transform_depth, params->wavelet_filter_index, bpp));
}

// ... and into a v216, ARGB or AY64 output picture -- the > 8-bit formats, no prediction (the reference has no > 8-bit inter
// path) --, with x_combine's schro_frame_shift_right (schrodecoder.c:2013-2019) in the same call: schro_hip_iiwt_pack_wide_batch.
static int
inverse_iwt_transform_wide (SchroHipFrame * packed, SchroHipFrame * transform_frame, SchroHipParams * params, int shift, int bpp)
{
  SchroHipContext *ctx = frame_ctx (packed);
  SchroHipIwtPackWidePicture pic;
  SCHRO_HIP_TRY (fill_fused_picture (pic, packed, transform_frame, params, false,[](int) { return 0; }));
  pic.format = packed->format;
  pic.shift = shift;
  return stage_done (ctx, schro_hip_iiwt_pack_wide_batch (ctx, &pic, 1, params->transform_depth, params->wavelet_filter_index, bpp));
}

// the three fused calls behind one door: the destination's format chooses (shift: the wide formats'; prediction: the 8-bit ones')
static int
inverse_iwt_transform_fused (SchroHipFrame * packed, SchroHipFrame * transform_frame, SchroHipParams * params, SchroHipFrame * prediction,
    int shift)
{
  const bool pack8 = packed->format == SCHRO_HIP_FORMAT_YUYV || packed->format == SCHRO_HIP_FORMAT_UYVY || packed->format == SCHRO_HIP_FORMAT_AYUV;
  SCHRO_HIP_REQUIRE (pack8 || ((packed->format == SCHRO_HIP_FORMAT_v210 || is_wide_format (packed->format)) && !prediction),
      "inverse_iwt_transform_convert: the destination must be a YUYV, UYVY, AYUV or (without a prediction: the reference has no "
      "> 8-bit inter path) v210, v216, ARGB or AY64 frame");
  const int bpp = format_bpp (transform_frame->format);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "inverse_iwt_transform_convert: the transform frame must be s16 or s32");
  if (pack8)
    return inverse_iwt_transform_pack8 (packed, transform_frame, params, prediction, bpp);
  if (is_wide_format (packed->format))
    return inverse_iwt_transform_wide (packed, transform_frame, params, shift, bpp);
  SchroHipContext *ctx = frame_ctx (packed);
  SchroHipIwtPackPicture pic;
  SCHRO_HIP_TRY (fill_fused_picture (pic, packed, transform_frame, params, true,[](int) { return 0; }));
  return stage_done (ctx, schro_hip_iiwt_pack_v210_batch (ctx, &pic, 1, params->transform_depth, params->wavelet_filter_index, bpp));
}

int
schro_frame_inverse_iwt_transform_combine_convert_hip (SchroHipFrame * packed, SchroHipFrame * transform_frame, SchroHipParams * params,
    SchroHipFrame * prediction)
{
  SCHRO_HIP_REQUIRE (packed && transform_frame && params && frame_ctx (packed) && transform_frame->domain == packed->domain,
      "inverse_iwt_transform_convert: the packed frame and the transform frame must live in the same device domain");
  return inverse_iwt_transform_fused (packed, transform_frame, params, prediction, 0);
}

int
schro_frame_inverse_iwt_transform_convert_hip (SchroHipFrame * packed, SchroHipFrame * transform_frame, SchroHipParams * params)
{
  return schro_frame_inverse_iwt_transform_combine_convert_hip (packed, transform_frame, params, nullptr);
}

// the whole non-reference intra tail of x_combine (schrodecoder.c:2009-2021: schro_frame_shift_right where the stream's bit
// depth exceeds the output picture's, then schro_frame_convert) behind x_wavelet_transform, in one stage call
int
schro_frame_inverse_iwt_transform_shift_convert_hip (SchroHipFrame * packed, SchroHipFrame * transform_frame, SchroHipParams * params, int shift)
{
  SCHRO_HIP_REQUIRE (packed && transform_frame && params && frame_ctx (packed) && transform_frame->domain == packed->domain,
      "inverse_iwt_transform_shift_convert: the packed frame and the transform frame must live in the same device domain");
  SCHRO_HIP_REQUIRE (shift == 0 || is_wide_format (packed->format), "inverse_iwt_transform_shift_convert: a shift of %d with a format "
      "other than v216 / ARGB / AY64 (schro_frame_inverse_iwt_transform_hip + schro_hipframe_shift_right + schro_hipframe_convert)", shift);
  return inverse_iwt_transform_fused (packed, transform_frame, params, nullptr, shift);
}

int
schro_hip_decode_lowdelay_transform_data (SchroHipFrame * transform_frame, const void *slices,
    size_t slices_bytes, const SchroHipLowDelayParams * params)
{
  SCHRO_HIP_REQUIRE (transform_frame && frame_ctx (transform_frame) && slices && params,
      "decode_lowdelay_transform_data: bad arguments");
  SchroHipContext *ctx = frame_ctx (transform_frame);
  const int bpp = format_bpp (transform_frame->format);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "decode_lowdelay_transform_data: the frame must be s16 or s32");
  for (int k = 0; k < 3; k++)
    SCHRO_HIP_TRY (require_holds ("decode_lowdelay_transform_data", k, transform_frame->components[k], iwt_size (params, k), 0));
  // picture->lowdelay_buffer goes to the device as it is: compressed
  SyncBlock blk (ctx, 0, 0, slices_bytes);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  int r = 0;
  if (hipMemcpyAsync (blk.part (kBytes), slices, slices_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "decode_lowdelay_transform_data: copy of %zu bytes failed", slices_bytes);
  if (!r) {
    SchroHipLowDelayPicture pic;
    pic.slices = (const uint8_t *) blk.part (kBytes);
    pic.slices_bytes = slices_bytes;
    for (int k = 0; k < 3; k++) {
      pic.comp[k] = transform_frame->components[k].data;
      pic.stride[k] = transform_frame->components[k].stride;
    }
    r = schro_hip_lowdelay_batch (ctx, &pic, 1, params, bpp);
  }
  return blk.finish (r);
}

// schro_encoder_encode_lowdelay_transform_data (schrolowdelay.c:1150-1200) with frame->iwt_frame on the device: the bytes
// the reference appends to frame->pack come back to the host, compressed, instead of 2 bytes per coefficient.
int
schro_hip_encode_lowdelay_transform_data (const SchroHipFrame * iwt_frame, void *slices, size_t slices_bytes,
    const SchroHipLowDelayParams * params, uint8_t * base_index, int *overruns)
{
  SCHRO_HIP_REQUIRE (iwt_frame && frame_ctx (iwt_frame) && slices && params,
      "encode_lowdelay_transform_data: bad arguments (the iwt frame must be a device frame)");
  SchroHipContext *ctx = frame_ctx (iwt_frame);
  const int bpp = format_bpp (iwt_frame->format);
  SCHRO_HIP_REQUIRE (bpp != 4, "encode_lowdelay_transform_data: s32 slices are not encoded (the reference's encoder is s16)");
  SCHRO_HIP_REQUIRE (bpp == 2, "encode_lowdelay_transform_data: the frame must be s16");
  for (int k = 0; k < 3; k++)
    SCHRO_HIP_TRY (require_holds ("encode_lowdelay_transform_data", k, iwt_frame->components[k], iwt_size (params, k), 0));
  SCHRO_HIP_REQUIRE (params->n_horiz_slices > 0 && params->n_vert_slices > 0
      && (int64_t) params->n_horiz_slices * params->n_vert_slices < (1 << 24), "encode_lowdelay_transform_data: bad slice counts");
  const size_t nslices = (size_t) params->n_horiz_slices * params->n_vert_slices;
  enum { kSlices, kIndex, kCount };
  SyncBlock blk (ctx, slices_bytes, nslices, 16, 16);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  SchroHipLowDelayEncodePicture pic;
  for (int k = 0; k < 3; k++) {
    pic.comp[k] = iwt_frame->components[k].data;
    pic.stride[k] = iwt_frame->components[k].stride;
  }
  pic.slices = (uint8_t *) blk.part (kSlices);
  pic.slices_bytes = slices_bytes;
  pic.base_index = (uint8_t *) blk.part (kIndex);
  pic.overruns = (uint32_t *) blk.part (kCount);
  int r = schro_hip_lowdelay_encode_batch (ctx, &pic, 1, params, bpp);
  uint32_t count = 0;
  if (!r && (hipMemcpyAsync (slices, blk.part (kSlices), slices_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess
          || (base_index && hipMemcpyAsync (base_index, blk.part (kIndex), nslices, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
          || hipMemcpyAsync (&count, blk.part (kCount), sizeof (count), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
    r = set_error (SCHRO_HIP_EDEVICE, "encode_lowdelay_transform_data: copy of %zu bytes failed", slices_bytes);
  r = blk.finish (r);
  if (!r && overruns)
    *overruns = (int) count;
  return r;
}

// schro_encoder_encode_transform_data (schroencoder.c:3462-3483) for params->is_noarith with frame->quant_frame on the
// device: the bytes the reference appends to frame->pack come back to the host instead of the quant frame.
int
schro_hip_encode_transform_data_noarith (const SchroHipFrame * quant_frame, const SchroHipParams * params,
    const int *const quant_indices[3], void *out, size_t capacity, size_t *bytes,
    int subband_bits[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS], int false_zero[2])
{
  const char *who = "encode_transform_data_noarith";
  SCHRO_HIP_REQUIRE (quant_frame && frame_ctx (quant_frame) && params && quant_indices && bytes && (out || capacity == 0),
      "%s: bad arguments (the quant frame must be a device frame)", who);
  SchroHipContext *ctx = frame_ctx (quant_frame);
  const int bpp = format_bpp (quant_frame->format);
  SCHRO_HIP_REQUIRE ((bpp == 2 || bpp == 4) && !(quant_frame->format & 0x100), "%s: the frame must be a planar s16 or s32 frame", who);
  const int depth = params->transform_depth;
  SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "%s: transform_depth %d", who, depth);
  SchroHipNoarithPicture pic;
  fill_noarith_header (pic, params);
  std::vector < SchroHipCodeblock > recs[3];
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & q = quant_frame->components[k];
    const IwtSize s = iwt_size (params, k);
    SCHRO_HIP_REQUIRE (quant_indices[k], "%s: component %d has no quant indices", who, k);
    SCHRO_HIP_TRY (require_holds (who, k, q, s, bpp));
    SCHRO_HIP_TRY (layout_records (who, k, s, params, q.stride, bpp, recs[k]));
    SCHRO_HIP_TRY (set_quant_indices (who, k, recs[k], quant_indices[k]));
    pic.quant[k] = q.data;
    pic.bytes[k] = (size_t) q.stride * (size_t) s.h;
    pic.stride[k] = q.stride;
    pic.iwt_width[k] = s.w;
    pic.iwt_height[k] = s.h;
    pic.codeblocks[k] = recs[k].data ();
    pic.ncodeblocks[k] = (int) recs[k].size ();
  }
  SyncBlock blk (ctx, kResultFront, 0, capacity);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  pic.result = (SchroHipNoarithResult *) blk.part (kFront);
  pic.out = (uint8_t *) blk.part (kBytes);
  pic.capacity = capacity;
  int r = schro_hip_noarith_encode_batch (ctx, &pic, 1, bpp);
  SchroHipNoarithResult res;
  memset (&res, 0, sizeof (res));
  if (!r && hipMemcpyAsync (&res, blk.part (kFront), sizeof (res), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the result failed", who);
  const size_t take = blk.wait () ? 0 : std::min ((size_t) res.bytes, capacity);
  if (!r && take) {
    if (hipMemcpyAsync (out, blk.part (kBytes), take, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of %zu bytes failed", who, take);
    blk.wait ();
  }
  if ((r = blk.finish (r)))
    return r;
  *bytes = res.bytes;
  if (subband_bits)
    for (int k = 0; k < 3; k++)
      for (int i = 0; i < SCHRO_HIP_NOARITH_MAX_SUBBANDS; i++)
        subband_bits[k][i] = (int) res.subband_bits[k][i];
  if (false_zero) {
    false_zero[0] = (int) res.false_zero_codeblocks;
    false_zero[1] = (int) res.false_zero_subbands;
  }
  if (res.overrun)
    return set_status (SCHRO_HIP_ENOMEM, "%s: the picture takes %u bytes, the buffer holds %zu", who, res.bytes, capacity);
  return 0;
}

// The motion data of a noarith picture (schroencoder.c:2505-2515): the host field goes up, the bytes the reference
// appends to frame->pack come back.
int
schro_hip_encode_motion_data_noarith (SchroHipContext * ctx, const SchroHipMotion * motion, const SchroHipParams * params,
    void *out, size_t capacity, size_t *bytes, int section_bytes[SCHRO_HIP_MOTION_SECTIONS], SchroHipMotionEncodeResult * result)
{
  const char *who = "encode_motion_data_noarith";
  SCHRO_HIP_REQUIRE (ctx && motion && motion->motion_vectors && params && bytes && (out || capacity == 0), "%s: bad arguments", who);
  const int64_t bound = schro_hip_motion_encode_bound (params->x_num_blocks, params->y_num_blocks, params->num_refs, params->have_global_motion);
  if (bound < 0)
    return (int) bound;
  capacity = std::min (capacity, (size_t) bound);
  const size_t field_bytes = (size_t) params->x_num_blocks * params->y_num_blocks * kMvBytes;
  SyncBlock blk (ctx, kResultFront, field_bytes, capacity);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  SchroHipMotionEncodePicture pic;
  memset (&pic, 0, sizeof (pic));
  pic.motion = blk.part (kField);
  pic.x_num_blocks = params->x_num_blocks;
  pic.y_num_blocks = params->y_num_blocks;
  pic.num_refs = params->num_refs;
  pic.have_global_motion = params->have_global_motion;
  pic.out = (uint8_t *) blk.part (kBytes);
  pic.capacity = capacity;
  pic.result = (SchroHipMotionEncodeResult *) blk.part (kFront);
  int r = 0;
  // (the batch call's layout launch writes every word of the result; cleared here so that a launch that did not run
  // reports no bytes instead of what the allocation held)
  if (hipMemsetAsync (blk.part (kFront), 0, kResultFront, ctx->stream) != hipSuccess
      || hipMemcpyAsync (blk.part (kField), motion->motion_vectors, field_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the field failed", who);
  if (!r)
    r = schro_hip_motion_encode_batch (ctx, &pic, 1);
  SchroHipMotionEncodeResult res;
  memset (&res, 0, sizeof (res));
  if (!r && hipMemcpyAsync (&res, blk.part (kFront), sizeof (res), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the result failed", who);
  const size_t take = blk.wait () ? 0 : std::min ((size_t) res.bytes, capacity);
  if (!r && take) {
    if (hipMemcpyAsync (out, blk.part (kBytes), take, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of %zu bytes failed", who, take);
    blk.wait ();
  }
  if ((r = blk.finish (r)))
    return r;
  *bytes = res.bytes;
  if (section_bytes)
    for (int s = 0; s < SCHRO_HIP_MOTION_SECTIONS; s++)
      section_bytes[s] = (int) res.section_bytes[s];
  if (result)
    *result = res;
  if (res.overrun)
    return set_status (SCHRO_HIP_ENOMEM, "%s: the picture takes %u bytes, the buffer holds %zu", who, res.bytes, capacity);
  return 0;
}

// The way back (schrodecoder.c:2531-2814): the host bytes go up, the host field and the result come back.
int
schro_hip_decode_motion_data_noarith (SchroHipContext * ctx, const void *data, size_t length, const SchroHipParams * params,
    SchroHipMotion * motion, SchroHipMotionDecodeResult * result)
{
  const char *who = "decode_motion_data_noarith";
  SCHRO_HIP_REQUIRE (ctx && (data || length == 0) && params && motion && motion->motion_vectors, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (params->x_num_blocks > 0 && params->y_num_blocks > 0 && params->x_num_blocks <= kMaxMotionBlocks
      && params->y_num_blocks <= kMaxMotionBlocks, "%s: %d x %d blocks", who, params->x_num_blocks, params->y_num_blocks);
  SCHRO_HIP_REQUIRE (length < ((size_t) 1 << 29), "%s: %zu bytes (below 2^29)", who, length);
  const size_t field_bytes = (size_t) params->x_num_blocks * params->y_num_blocks * kMvBytes;
  SyncBlock blk (ctx, kResultFront, field_bytes, length);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  SchroHipMotionDecodePicture pic;
  memset (&pic, 0, sizeof (pic));
  pic.data = (const uint8_t *) blk.part (kBytes);
  pic.data_bytes = length;
  pic.x_num_blocks = params->x_num_blocks;
  pic.y_num_blocks = params->y_num_blocks;
  pic.num_refs = params->num_refs;
  pic.have_global_motion = params->have_global_motion;
  pic.motion = blk.part (kField);
  pic.result = (SchroHipMotionDecodeResult *) blk.part (kFront);
  int r = 0;
  if (length && hipMemcpyAsync (blk.part (kBytes), data, length, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the bytes failed", who);
  if (!r)
    r = schro_hip_motion_decode_batch (ctx, &pic, 1);
  SchroHipMotionDecodeResult res;
  memset (&res, 0, sizeof (res));
  if (!r && (hipMemcpyAsync (&res, blk.part (kFront), sizeof (res), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess
          || hipMemcpyAsync (motion->motion_vectors, blk.part (kField), field_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the field failed", who);
  if ((r = blk.finish (r)))
    return r;
  if (result)
    *result = res;
  return 0;
}

// The same for an arithmetic-coded picture.
int
schro_hip_decode_motion_data_arith (SchroHipContext * ctx, const void *data, size_t length, const SchroHipParams * params,
    SchroHipMotion * motion, SchroHipMotionArithDecodeResult * result)
{
  const char *who = "decode_motion_data_arith";
  SCHRO_HIP_REQUIRE (ctx && (data || length == 0) && params && motion && motion->motion_vectors, "%s: bad arguments", who);
  SCHRO_HIP_REQUIRE (!params->is_noarith, "%s: the picture is noarith (schro_hip_decode_motion_data_noarith)", who);
  SCHRO_HIP_REQUIRE (params->x_num_blocks > 0 && params->y_num_blocks > 0 && params->x_num_blocks <= kMaxMotionBlocks
      && params->y_num_blocks <= kMaxMotionBlocks, "%s: %d x %d blocks", who, params->x_num_blocks, params->y_num_blocks);
  SCHRO_HIP_REQUIRE (length < ((size_t) 1 << 29), "%s: %zu bytes (below 2^29)", who, length);
  const size_t field_bytes = (size_t) params->x_num_blocks * params->y_num_blocks * kMvBytes;
  SyncBlock blk (ctx, kResultFront, field_bytes, length);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  SchroHipMotionArithDecodePicture pic;
  memset (&pic, 0, sizeof (pic));
  pic.data = (const uint8_t *) blk.part (kBytes);
  pic.data_bytes = length;
  pic.x_num_blocks = params->x_num_blocks;
  pic.y_num_blocks = params->y_num_blocks;
  pic.num_refs = params->num_refs;
  pic.have_global_motion = params->have_global_motion;
  pic.motion = blk.part (kField);
  pic.result = (SchroHipMotionArithDecodeResult *) blk.part (kFront);
  int r = 0;
  if (length && hipMemcpyAsync (blk.part (kBytes), data, length, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the bytes failed", who);
  if (!r)
    r = schro_hip_motion_arith_decode_batch (ctx, &pic, 1);
  SchroHipMotionArithDecodeResult res;
  memset (&res, 0, sizeof (res));
  if (!r && (hipMemcpyAsync (&res, blk.part (kFront), sizeof (res), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess
          || hipMemcpyAsync (motion->motion_vectors, blk.part (kField), field_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the field failed", who);
  if ((r = blk.finish (r)))
    return r;
  if (result)
    *result = res;
  return 0;
}

// r05 -- schro_decoder_decode_subband's data-parallel half on the device, behind the frame layer: the picture arrives
// as codeblock records + quantised values (include/schro_hip.h), leaves as the dense transform frame x_wavelet_transform
// reads.  Reference: schrodecoder.c:3525-3640 (the codeblock loop), :3311-3322 (zero codeblocks), :3060-3083 / :3400-3451
// (dequantisation), :3629-3636 + :3219-3277 (DC prediction of an intra picture's LL bands), :3280-3293 (codeblock counts).
int
schro_hipframe_dequantise (SchroHipFrame * transform_frame, const SchroHipQuantisedPicture * q, SchroHipParams * params)
{
  SCHRO_HIP_REQUIRE (transform_frame && frame_ctx (transform_frame) && q && params, "hipframe_dequantise: bad arguments "
      "(the transform frame must be a device frame)");
  SchroHipContext *ctx = frame_ctx (transform_frame);
  const int bpp = format_bpp (transform_frame->format);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "hipframe_dequantise: the transform frame must be s16 or s32");
  (void) hipSetDevice (ctx->device);
  const int arith = params->is_noarith && bpp == 2 ? 1 : 0;
  const int intra = params->num_refs == 0;
  SchroHipDequantPlane planes[3];
  size_t stage_bytes = 0;
  for (int k = 0; k < 3; k++) {
    SCHRO_HIP_REQUIRE (q->codeblocks[k] && q->ncodeblocks[k] > 0 && (q->values[k] || q->values_bytes[k] == 0),
        "hipframe_dequantise: component %d has no codeblock records (or values_bytes without values)", k);
    stage_bytes += (q->values_bytes[k] + 255) & ~(size_t) 255;
    // r06: the records come, in the end, from the bitstream -- every codeblock lies inside its component
    // and its values inside the blob, or nothing is launched (two cheap loops over records the plan compare reads anyway)
    const SchroHipFrameData & comp = transform_frame->components[k];
    const long long comp_bytes = comp.length > 0 ? (long long) comp.length : (long long) comp.stride * comp.height;
    for (int n = 0; n < q->ncodeblocks[k]; n++) {
      const SchroHipCodeblock & cb = q->codeblocks[k][n];
      const long long row = (long long) cb.width * bpp;
      SCHRO_HIP_REQUIRE (cb.width >= 0 && cb.height >= 0, "hipframe_dequantise: component %d, codeblock %d has a negative size", k, n);
      if (cb.width == 0 || cb.height == 0)      // (an empty codeblock of a tiny sub-band: nothing is read or written)
        continue;
      SCHRO_HIP_REQUIRE (cb.dst_offset >= 0 && cb.dst_stride >= comp.stride && comp.stride > 0
          && cb.dst_stride % comp.stride == 0 && cb.dst_offset % bpp == 0
          && (long long) (cb.dst_offset % comp.stride) + row <= (long long) comp.stride
          && (long long) cb.dst_offset + (long long) (cb.height - 1) * cb.dst_stride + row <= comp_bytes,
          "hipframe_dequantise: component %d, codeblock %d (%d x %d at byte %d, pitch %d) does not lie inside the transform frame's "
          "component (%d x %d, stride %d)", k, n, cb.width, cb.height, cb.dst_offset, cb.dst_stride, comp.width, comp.height, comp.stride);
      SCHRO_HIP_REQUIRE (cb.src_offset < 0 || ((cb.src_bytes == 1 || cb.src_bytes == 2 || cb.src_bytes == 4)
              && (unsigned long long) cb.src_offset + (unsigned long long) cb.width * cb.height * cb.src_bytes <= (unsigned long long) q->values_bytes[k]),
          "hipframe_dequantise: component %d, codeblock %d: its values (%d bytes each, from byte %d) do not lie inside the %zu bytes of values",
          k, n, (int) cb.src_bytes, cb.src_offset, (size_t) q->values_bytes[k]);
    }
  }
  // host-side values: staged in a buffer of the selected queue (the queue's order keeps a later call's copy behind this
  // call's kernel); a host that pipelines uploads the picture's blob itself, on the copy queue, and passes device pointers
  char *stage = nullptr;
  if (!q->values_on_device && stage_bytes) {
    void *&buf = ctx->dq_stage_q[ctx->cur];
    size_t & size = ctx->dq_stage_size_q[ctx->cur];
    if (size < stage_bytes)     // (a quarter of headroom: pictures of one stream differ a little)
      SCHRO_HIP_TRY (grow_block (ctx, buf, size, stage_bytes + stage_bytes / 4));
    stage = (char *) buf;
  }
  size_t off = 0;
  for (int k = 0; k < 3; k++) {
    SchroHipDequantPlane & pl = planes[k];
    pl.dst = transform_frame->components[k].data;
    pl.codeblocks = q->codeblocks[k];
    pl.ncodeblocks = q->ncodeblocks[k];
    pl.is_intra = intra;
    if (q->values_on_device || !q->values_bytes[k]) {
      pl.values = q->values[k];
    } else {
      SCHRO_HIP_CHECK (hipMemcpyAsync (stage + off, q->values[k], q->values_bytes[k], hipMemcpyHostToDevice, ctx->stream));
      pl.values = stage + off;
      off += (q->values_bytes[k] + 255) & ~(size_t) 255;
    }
  }
  // the plan of this picture geometry: kept while pictures of the same geometry follow each other
  int r = SCHRO_HIP_EINVAL;
  if (ctx->frame_dq_plan)
    r = schro_hip_dequant_plan_matches (ctx->frame_dq_plan, planes, 3, bpp, arith) ? 0 : SCHRO_HIP_EINVAL;
  if (r) {
    if (ctx->frame_dq_plan)
      schro_hip_dequant_plan_free (ctx->frame_dq_plan);
    ctx->frame_dq_plan = schro_hip_dequant_plan_new (ctx, planes, 3, bpp, arith);
    if (!ctx->frame_dq_plan)
      return SCHRO_HIP_EINVAL;
  }
  r = schro_hip_dequant_plan_run (ctx->frame_dq_plan, planes, 3);
  if (!r && intra) {
    SchroHipDcPlane ll[3];
    ll_planes (ll, transform_frame, params);
    r = schro_hip_dc_predict_batch (ctx, ll, 3, bpp);
  }
  return stage_done (ctx, r);
}

// schro_decoder_parse_transform_data + schro_decoder_decode_transform_data for params->is_noarith: the picture's bytes go
// up instead of the entropy-decoded values; the frame is left as schro_hipframe_dequantise leaves it.
int
schro_hipframe_decode_transform_data_noarith (SchroHipFrame * transform_frame, const uint8_t * host_data, size_t length,
    SchroHipParams * params, int *compat_quant_offset, SchroHipNoarithDecodeResult * result)
{
  const char *who = "hipframe_decode_transform_data_noarith";
  SCHRO_HIP_REQUIRE (transform_frame && frame_ctx (transform_frame) && params && compat_quant_offset && result
      && (host_data || length == 0), "%s: bad arguments (the transform frame must be a device frame)", who);
  SchroHipContext *ctx = frame_ctx (transform_frame);
  const int bpp = format_bpp (transform_frame->format);
  SCHRO_HIP_REQUIRE ((bpp == 2 || bpp == 4) && !(transform_frame->format & 0x100), "%s: the frame must be a planar s16 or s32 frame", who);
  const int depth = params->transform_depth;
  SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "%s: transform_depth %d", who, depth);
  SCHRO_HIP_REQUIRE (length < ((size_t) 1 << 29), "%s: %zu bytes (below 2^29)", who, length);
  (void) hipSetDevice (ctx->device);
  const int intra = params->num_refs == 0;
  SchroHipNoarithDecodePicture pic;
  fill_noarith_header (pic, params);
  pic.is_intra = intra;
  pic.compat_quant_offset = *compat_quant_offset != 0;
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & c = transform_frame->components[k];
    const IwtSize s = iwt_size (params, k);
    SCHRO_HIP_TRY (require_holds (who, k, c, s, bpp));
    pic.coeffs[k] = c.data;
    pic.bytes[k] = (size_t) c.stride * (size_t) s.h;
    pic.stride[k] = c.stride;
    pic.iwt_width[k] = s.w;
    pic.iwt_height[k] = s.h;
  }
  SyncBlock blk (ctx, kNoarithDecodeFront, 0, length);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  pic.result = (SchroHipNoarithDecodeResult *) blk.part (kFront);
  pic.data = (const uint8_t *) blk.part (kBytes);
  pic.data_bytes = length;
  int r = 0;
  if (length && hipMemcpyAsync (blk.part (kBytes), host_data, length, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of %zu bytes failed", who, length);
  if (!r)
    r = schro_hip_noarith_decode_batch (ctx, &pic, 1, bpp);
  memset (result, 0, sizeof (*result));
  if (!r && hipMemcpyAsync (result, blk.part (kFront), sizeof (*result), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the result failed", who);
  if ((r = blk.finish (r)))
    return r;
  if (result->error)
    return set_status (SCHRO_HIP_EINVAL, "%s: quant index above 60 in the header of component %u, sub-band %u", who,
        result->first_error / SCHRO_HIP_NOARITH_MAX_SUBBANDS, result->first_error % SCHRO_HIP_NOARITH_MAX_SUBBANDS);
  *compat_quant_offset = (int) result->compat_quant_offset;
  if (intra) {
    SchroHipDcPlane ll[3];
    ll_planes (ll, transform_frame, params);
    r = schro_hip_dc_predict_batch (ctx, ll, 3, bpp);
  }
  return stage_done (ctx, r);
}

// ... and for an arithmetic-coded picture (schro_hip_arith_decode_batch)
static_assert (sizeof (SchroHipArithDecodeResult) <= kNoarithDecodeFront, "the result sits in front of the bytes");
int
schro_hipframe_decode_transform_data_arith (SchroHipFrame * transform_frame, const uint8_t * host_data, size_t length,
    SchroHipParams * params, int *compat_quant_offset, SchroHipArithDecodeResult * result)
{
  const char *who = "hipframe_decode_transform_data_arith";
  SCHRO_HIP_REQUIRE (transform_frame && frame_ctx (transform_frame) && params && compat_quant_offset && result
      && (host_data || length == 0), "%s: bad arguments (the transform frame must be a device frame)", who);
  SCHRO_HIP_REQUIRE (!params->is_noarith && !params->is_lowdelay, "%s: the picture is %s, not arithmetic-coded core syntax", who,
      params->is_lowdelay ? "low delay" : "noarith (VLC)");
  SchroHipContext *ctx = frame_ctx (transform_frame);
  const int bpp = format_bpp (transform_frame->format);
  SCHRO_HIP_REQUIRE ((bpp == 2 || bpp == 4) && !(transform_frame->format & 0x100), "%s: the frame must be a planar s16 or s32 frame", who);
  const int depth = params->transform_depth;
  SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "%s: transform_depth %d", who, depth);
  SCHRO_HIP_REQUIRE (length < ((size_t) 1 << 29), "%s: %zu bytes (below 2^29)", who, length);
  (void) hipSetDevice (ctx->device);
  const int intra = params->num_refs == 0;
  SchroHipArithDecodePicture pic;
  fill_noarith_header (pic, params);
  pic.is_intra = intra;
  pic.compat_quant_offset = *compat_quant_offset != 0;
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & c = transform_frame->components[k];
    const IwtSize s = iwt_size (params, k);
    SCHRO_HIP_TRY (require_holds (who, k, c, s, bpp));
    pic.coeffs[k] = c.data;
    pic.bytes[k] = (size_t) c.stride * (size_t) s.h;
    pic.stride[k] = c.stride;
    pic.iwt_width[k] = s.w;
    pic.iwt_height[k] = s.h;
  }
  SyncBlock blk (ctx, kNoarithDecodeFront, 0, length);
  if (!blk.d)
    return SCHRO_HIP_ENOMEM;
  pic.result = (SchroHipArithDecodeResult *) blk.part (kFront);
  pic.data = (const uint8_t *) blk.part (kBytes);
  pic.data_bytes = length;
  int r = 0;
  if (length && hipMemcpyAsync (blk.part (kBytes), host_data, length, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of %zu bytes failed", who, length);
  if (!r)
    r = schro_hip_arith_decode_batch (ctx, &pic, 1, bpp);
  memset (result, 0, sizeof (*result));
  if (!r && hipMemcpyAsync (result, blk.part (kFront), sizeof (*result), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    r = set_error (SCHRO_HIP_EDEVICE, "%s: copy of the result failed", who);
  if ((r = blk.finish (r)))
    return r;
  if (result->error)
    return set_status (SCHRO_HIP_EINVAL, "%s: quant index above 60 in the header of component %u, sub-band %u", who,
        result->first_error / SCHRO_HIP_NOARITH_MAX_SUBBANDS, result->first_error % SCHRO_HIP_NOARITH_MAX_SUBBANDS);
  *compat_quant_offset = (int) result->compat_quant_offset;
  if (intra) {
    SchroHipDcPlane ll[3];
    ll_planes (ll, transform_frame, params);
    r = schro_hip_dc_predict_batch (ctx, ll, 3, bpp);
  }
  return stage_done (ctx, r);
}

int
schro_upsampled_hipframe_upsample (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (dest) && src->domain == dest->domain
      && dest->is_upsampled && !src->is_upsampled && format_bpp (src->format) == 1,
      "upsampled_hipframe_upsample: bad arguments");
  if (dest->upsample_done)      // schroframe.c:2006-2009
    return 0;
  SchroHipUpsamplePlane planes[3];
  const bool pair = dest->is_upsampled == 2;    // chroma as one pair image
  for (int k = 0; k < 3; k++) {
    SCHRO_HIP_REQUIRE (dest->components[k].width == src->components[k].width
        && dest->components[k].height == src->components[k].height,
        "upsampled_hipframe_upsample: size mismatch");
    planes[k].src = (const uint8_t *) src->components[k].data;
    planes[k].src_stride = src->components[k].stride;
    planes[k].dst = (uint8_t *) dest->components[k].data;
    planes[k].dst_stride = dest->components[k].stride;
    planes[k].width = src->components[k].width;
    planes[k].height = src->components[k].height;
    planes[k].src_v = nullptr;
    planes[k].src_v_stride = 0;
  }
  if (pair) {
    planes[1].src_v = planes[2].src;
    planes[1].src_v_stride = planes[2].src_stride;
  }
  int r = stage_done (frame_ctx (dest), schro_hip_upsample_batch (frame_ctx (dest), planes, pair ? 2 : 3));
  if (!r)
    dest->upsample_done = 1;
  return r;
}

// schro_upsampled_gpuframe_upsample (SchroFrame *) (schrogpuframe.h:29): one argument, the upsampled
// frame, whose integer-pel source is the frame it keeps in virt_frame1
int
schro_upsampled_hipframe_upsample_inplace (SchroHipFrame * frame)
{
  SCHRO_HIP_REQUIRE (frame && frame->is_upsampled && frame->virt_frame1,
      "upsampled_hipframe_upsample_inplace: needs an upsampled frame with its source frame in virt_frame1");
  return schro_upsampled_hipframe_upsample (frame, frame->virt_frame1);
}

int
schro_motion_render_hip (SchroHipMotion * motion, SchroHipFrame * dest, SchroHipFrame * addframe, int add,
    SchroHipFrame * output_frame)
{
  // add == FALSE (r04): the prediction alone into `dest`, a u8 device frame -- schro_motion_render_cuda (motion,
  // mc_tmp_frame) (schrodecoder.c:1759) --, for schro_frame_inverse_iwt_transform_combine_hip to add.  Else `dest`
  // is the CPU path's s16 scratch frame and not used: the accumulator lives in LDS here.
  // r06: ... or an S16 device frame, which receives the prediction - 128 -- the literal contract of
  // schro_motion_render_cuda (motion, mc_tmp_frame) (schrocuda.h:13, schrodecoder.c:1742-1760) and of the CPU call's
  // add = FALSE (orc_rrshift6_sub_s16_2d's d2, schromotion8.c:896-899): schro_hipframe_add (frame, mc_tmp_frame) and
  // schro_hipframe_convert then finish the picture as schrodecoder.c:1908-1910, 2011 do.  Any weights, any DC values.
  bool s16_dest = false;
  if (!add) {
    SCHRO_HIP_REQUIRE (dest && frame_ctx (dest) && (format_bpp (dest->format) == 1 || format_bpp (dest->format) == 2) && !addframe,
        "motion_render: add = FALSE renders the prediction into `dest`, a u8 or s16 device frame (addframe NULL)");
    output_frame = dest;
    s16_dest = format_bpp (dest->format) == 2;
  }
  // addframe NULL: nothing to add -- a zero_residual picture has no frame (schrodecoder.c:1800, :1861,
  // :1904-1906: the GPU paths take mc_tmp_frame as the combined frame); the prediction alone is clamped
  SCHRO_HIP_REQUIRE (motion && motion->params && motion->src1 && motion->motion_vectors
      && output_frame && frame_ctx (output_frame) && (!addframe || addframe->domain == output_frame->domain),
      "motion_render: bad arguments");
  const SchroHipParams *p = motion->params;
  if (p->have_global_motion)    // schromotion.c:113-118 routes this to another renderer
    return set_error (SCHRO_HIP_EUNSUPPORTED, "motion_render: global motion is not supported");
  SchroHipContext *ctx = frame_ctx (output_frame);
  const int upsampled = p->mv_precision > 0;
  SCHRO_HIP_REQUIRE ((motion->src1->is_upsampled != 0) == upsampled
      && (!motion->src2 || motion->src2->is_upsampled == motion->src1->is_upsampled),
      "motion_render: references must be %s for mv_precision %d",
      upsampled ? "upsampled frames" : "plain frames", p->mv_precision);
  if (p->num_refs == 1)         // schromotion8.c:711-713
    SCHRO_HIP_REQUIRE (p->picture_weight_2 == 1, "motion_render: one reference needs picture_weight_2 == 1");

  // SchroMotionVector array -> device (schrogpumotion.c:68-120 did a repack; the kernel reads the
  // 20-byte records as they are).  r04: through the context's pinned table mirrors (push_big_table: one
  // memcpy into pinned memory + an asynchronous copy on the queue, buffers used in turn) -- no allocation,
  // no pageable-memory copy and no wait per call; a motion whose vectors are ALREADY on the device (a
  // host that uploaded them on the copy queue) is used where it is.
  (void) hipSetDevice (ctx->device);
  size_t mv_bytes = (size_t) 20 * p->x_num_blocks * p->y_num_blocks;
  void *d_mvs = nullptr;
  // r05 -- the combine form routes itself.  A prediction that cannot be a u8 plane (weights with a gain above 1; a DC
  // block whose value lies outside [-128, 127]: the reference's s16 block arithmetic carries it, schromotion8.c:542-568,
  // and wraps) is answered BEFORE anything is launched: SCHRO_HIP_ENEEDS_RESIDUAL, and the caller runs the picture in
  // the residual order (schrodecoder.c:1742-1760's stages the other way round: INTEGRATION 3).  Vectors that are already
  // on the device cannot be looked at here; the launch flags them (schro_hip_obmc_batch, prediction_only).
  if (!add && !s16_dest && (p->picture_weight_1 < 0 || p->picture_weight_2 < 0
          || p->picture_weight_1 + p->picture_weight_2 > (1 << p->picture_weight_bits)))
    return set_status (SCHRO_HIP_ENEEDS_RESIDUAL, "motion_render (add = FALSE): picture weights %d, %d / 2^%d can predict beyond 8 bits: "
        "this picture takes the residual order", p->picture_weight_1, p->picture_weight_2, p->picture_weight_bits);
  {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes (&attr, motion->motion_vectors) == hipSuccess && attr.type == hipMemoryTypeDevice) {
      d_mvs = motion->motion_vectors;
    } else {
      (void) hipGetLastError ();        // (an ordinary host pointer is "invalid value" to the query)
      if (!add && !s16_dest) {
        // SchroMotionVector (schromotion.h:53-75): pred_mode in the two low bits of the first word, the DC
        // values as three int16 at byte 12.  (Blocks on the picture's rim store their DC as a uint8_t and would
        // fit; they are refused with the rest -- the residual order is exact for every picture.)
        const unsigned char *mvb = (const unsigned char *) motion->motion_vectors;
        const size_t nmv = (size_t) p->x_num_blocks * p->y_num_blocks;
        for (size_t i = 0; i < nmv; i++) {
          const unsigned char *r = mvb + 20 * i;
          if (r[0] & 3)
            continue;
          int16_t dc[3];
          memcpy (dc, r + 12, 6);
          if ((unsigned) (dc[0] + 128) > 255u || (unsigned) (dc[1] + 128) > 255u || (unsigned) (dc[2] + 128) > 255u)
            return set_status (SCHRO_HIP_ENEEDS_RESIDUAL, "motion_render (add = FALSE): block %zu has a DC value outside [-128, 127] "
                "(%d, %d, %d): its prediction does not fit 8 bits, this picture takes the residual order", i, dc[0], dc[1], dc[2]);
        }
      }
      int r = push_big_table (ctx, motion->motion_vectors, mv_bytes, &d_mvs);
      if (r)
        return r;
    }
  }
  SchroHipObmcPlane planes[3];
  const int res_bpp = addframe ? format_bpp (addframe->format) : 2;
  for (int k = 0; k < 3; k++) {
    SchroHipObmcPlane & pl = planes[k];
    memset (&pl, 0, sizeof (pl));
    pl.mvs = d_mvs;
    pl.x_num_blocks = p->x_num_blocks;
    pl.y_num_blocks = p->y_num_blocks;
    pl.xblen_luma = p->xblen_luma;
    pl.yblen_luma = p->yblen_luma;
    pl.xbsep_luma = p->xbsep_luma;
    pl.ybsep_luma = p->ybsep_luma;
    pl.mv_precision = p->mv_precision;
    pl.picture_weight_bits = p->picture_weight_bits;
    pl.picture_weight_1 = p->picture_weight_1;
    pl.picture_weight_2 = p->picture_weight_2;
    pl.chroma_h_shift = SCHRO_HIP_FORMAT_H_SHIFT (output_frame->format);
    pl.chroma_v_shift = SCHRO_HIP_FORMAT_V_SHIFT (output_frame->format);
    pl.component = k;
    pl.ref1 = (const uint8_t *) motion->src1->components[k].data;
    pl.ref1_stride = motion->src1->components[k].stride;
    if (motion->src2) {
      pl.ref2 = (const uint8_t *) motion->src2->components[k].data;
      pl.ref2_stride = motion->src2->components[k].stride;
    }
    if (addframe) {
      pl.residual = addframe->components[k].data;
      pl.residual_stride = addframe->components[k].stride;
    }
    pl.residual_bpp = res_bpp;
    pl.out = (uint8_t *) output_frame->components[k].data;
    pl.out_stride = output_frame->components[k].stride;
    pl.width = output_frame->components[k].width;
    pl.height = output_frame->components[k].height;
    if (s16_dest) {
      // (the reference hands over a frame of the transform's padded size; the picture is what the references cover)
      pl.width = std::min (pl.width, motion->src1->components[k].width);
      pl.height = std::min (pl.height, motion->src1->components[k].height);
    }
    pl.ref_pair = k && motion->src1->is_upsampled == 2;
    pl.prediction_only = add ? 0 : s16_dest ? 2 : 1;
  }
  return stage_done (ctx, schro_hip_obmc_batch (ctx, planes, 3));
}

int
schro_hipframe_convert (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (dest) && src->domain == dest->domain,
      "hipframe_convert: both frames must live in the same device domain");
  SchroHipContext *ctx = frame_ctx (dest);
  if (dest->format & 0x100) {
    // copy-out into a packed frame (schroframe.c:878-899, 943-968)
    const bool wide = is_wide_format (dest->format), v210 = dest->format == SCHRO_HIP_FORMAT_v210;
    SCHRO_HIP_REQUIRE (!(src->format & 0x100) && format_bpp (src->format)
        && (wide || v210 || format_bpp (src->format) == 1),
        "hipframe_convert: YUYV / UYVY / AYUV take a planar u8 source (convert to u8 first)");
    SchroHipPackPlane pl;
    for (int k = 0; k < 3; k++) {
      pl.src[k] = (const uint8_t *) src->components[k].data;
      pl.src_stride[k] = src->components[k].stride;
    }
    pl.src_width = src->width;
    pl.src_height = src->height;
    pl.src_h_shift = SCHRO_HIP_FORMAT_H_SHIFT (src->format);
    pl.src_v_shift = SCHRO_HIP_FORMAT_V_SHIFT (src->format);
    pl.dst = (uint8_t *) dest->components[0].data;
    pl.dst_stride = dest->components[0].stride;
    pl.width = dest->width;
    pl.height = dest->height;
    pl.format = dest->format;
    int r = wide ? schro_hip_pack_wide_batch (ctx, &pl, 1, format_bpp (src->format))
        : v210 ? schro_hip_pack_v210_batch (ctx, &pl, 1, format_bpp (src->format)) : schro_hip_pack_u8_batch (ctx, &pl, 1);
    return stage_done (ctx, r);
  }
  int sb = format_bpp (src->format), db = format_bpp (dest->format);
  if (db == 1 && (sb == 2 || sb == 4)) {
    SchroHipConvertPlane planes[3];
    common_planes (planes, dest, src);
    return stage_done (ctx, schro_hip_convert_u8_batch (ctx, planes, 3, sb));
  }
  if (db == sb) {
    (void) hipSetDevice (ctx->device);
    for (int k = 0; k < 3; k++) {
      int w = std::min (dest->components[k].width, src->components[k].width);
      int h = std::min (dest->components[k].height, src->components[k].height);
      SCHRO_HIP_CHECK (hipMemcpy2DAsync (dest->components[k].data, dest->components[k].stride,
              src->components[k].data, src->components[k].stride, (size_t) w * sb, h,
              hipMemcpyDeviceToDevice, ctx->stream));
    }
    return stage_done (ctx, 0);
  }
  return set_error (SCHRO_HIP_EUNSUPPORTED, "hipframe_convert: depth %d -> %d is not on the decode path",
      sb, db);
}

// The encoder-direction schro_frame_convert (schroframe.c:869-979; schroencoder.c:1053-1055, 2454): `src` a packed or a
// planar device frame, `dest` a planar one of any depth -- schro_hip_unpack_batch on the frames' components.
int
schro_hipframe_convert_input (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (dest) && src->domain == dest->domain,
      "hipframe_convert_input: both frames must live in the same device domain");
  SchroHipContext *ctx = frame_ctx (dest);
  SCHRO_HIP_REQUIRE (!(dest->format & 0x100) && format_bpp (dest->format), "hipframe_convert_input: the destination must be planar");
  SchroHipUnpackPicture pc;
  memset (&pc, 0, sizeof (pc));
  if (src->format & 0x100) {
    pc.format = src->format;
    pc.src[0] = src->components[0].data;
    pc.src_stride[0] = src->components[0].stride;
  } else {
    pc.src_bpp = format_bpp (src->format);
    pc.src_h_shift = SCHRO_HIP_FORMAT_H_SHIFT (src->format);
    pc.src_v_shift = SCHRO_HIP_FORMAT_V_SHIFT (src->format);
    for (int k = 0; k < 3; k++) {
      pc.src[k] = src->components[k].data;
      pc.src_stride[k] = src->components[k].stride;
    }
  }
  pc.src_width = src->width;
  pc.src_height = src->height;
  for (int k = 0; k < 3; k++) {
    pc.dst[k] = dest->components[k].data;
    pc.dst_stride[k] = dest->components[k].stride;
  }
  pc.dst_bpp = format_bpp (dest->format);
  pc.h_shift = SCHRO_HIP_FORMAT_H_SHIFT (dest->format);
  pc.v_shift = SCHRO_HIP_FORMAT_V_SHIFT (dest->format);
  pc.width = dest->width;
  pc.height = dest->height;
  return stage_done (ctx, schro_hip_unpack_batch (ctx, &pc, 1));
}

// An intra picture from the packed frame the application pushed to the coefficients in iwt_frame (s16 / s32, of the
// transform size): schro_hip_unpack_iwt_batch on the frames' components.
int
schro_hipframe_unpack_iwt_transform (SchroHipFrame * iwt_frame, SchroHipFrame * packed, const SchroHipParams * params, int picture_width,
    int picture_height)
{
  SCHRO_HIP_REQUIRE (iwt_frame && packed && params && frame_ctx (iwt_frame) && packed->domain == iwt_frame->domain,
      "hipframe_unpack_iwt_transform: both frames must live in the same device domain");
  SchroHipContext *ctx = frame_ctx (iwt_frame);
  const int bpp = format_bpp (iwt_frame->format);
  SCHRO_HIP_REQUIRE (!(iwt_frame->format & 0x100) && (bpp == 2 || bpp == 4), "hipframe_unpack_iwt_transform: the transform frame must be s16 or s32");
  SCHRO_HIP_REQUIRE (packed->format & 0x100, "hipframe_unpack_iwt_transform: the source must be a packed frame");
  SchroHipUnpackIwtPicture pc;
  memset (&pc, 0, sizeof (pc));
  pc.src = packed->components[0].data;
  pc.src_stride = packed->components[0].stride;
  pc.format = packed->format;
  pc.src_width = packed->width;
  pc.src_height = packed->height;
  pc.width = picture_width;
  pc.height = picture_height;
  pc.h_shift = SCHRO_HIP_FORMAT_H_SHIFT (iwt_frame->format);
  pc.v_shift = SCHRO_HIP_FORMAT_V_SHIFT (iwt_frame->format);
  pc.iwt_width = params->iwt_luma_width;
  pc.iwt_height = params->iwt_luma_height;
  for (int k = 0; k < 3; k++) {
    const IwtSize s = iwt_size (params, k);
    SCHRO_HIP_TRY (require_holds ("hipframe_unpack_iwt_transform", k, iwt_frame->components[k], s, 0));
    // (the plane layer's chroma planes are the luma size under the shifts, as the transform frame's components are)
    SCHRO_HIP_REQUIRE (!k || (s.w == (params->iwt_luma_width + pc.h_shift) >> pc.h_shift && s.h == (params->iwt_luma_height + pc.v_shift) >> pc.v_shift),
        "hipframe_unpack_iwt_transform: the chroma transform size %d x %d is not the luma size %d x %d under the frame's chroma shifts",
        s.w, s.h, params->iwt_luma_width, params->iwt_luma_height);
    pc.dst[k] = iwt_frame->components[k].data;
    pc.dst_stride[k] = iwt_frame->components[k].stride;
  }
  return stage_done (ctx, schro_hip_unpack_iwt_batch (ctx, &pc, 1, params->transform_depth, params->wavelet_filter_index, bpp));
}

// schro_gpuframe_add (dest, src) (schrogpuframe.h:18, call site schrodecoder.c:1908-1910) = schro_frame_add
// (schroframe.c:1000-1029), and schro_frame_subtract (dest, src) (schroframe.c:1031-1079): dest (s16) += or -= src (s16 | u8)
// over the components' common size
static int
add_or_subtract (SchroHipFrame * dest, SchroHipFrame * src, bool subtract)
{
  const char *word = subtract ? "subtract" : "add";
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (dest) && src->domain == dest->domain,
      "hipframe_%s: both frames must live in the same device domain", word);
  SCHRO_HIP_REQUIRE (!(dest->format & 0x100) && !(src->format & 0x100) && format_bpp (dest->format) == 2
      && (format_bpp (src->format) == 1 || format_bpp (src->format) == 2)
      && SCHRO_HIP_FORMAT_H_SHIFT (dest->format) == SCHRO_HIP_FORMAT_H_SHIFT (src->format)
      && SCHRO_HIP_FORMAT_V_SHIFT (dest->format) == SCHRO_HIP_FORMAT_V_SHIFT (src->format),
      "hipframe_%s: s16 %s s16 | u8 of the same chroma format (%s function unimplemented, schroframe.c:%d)", word,
      subtract ? "-=" : "+=", word, subtract ? 1078 : 1027);
  SchroHipConvertPlane planes[3];
  common_planes (planes, dest, src);
  SchroHipContext *ctx = frame_ctx (dest);
  return stage_done (ctx, subtract ? schro_hip_subtract_batch (ctx, planes, 3, format_bpp (src->format) == 1)
      : schro_hip_add_batch (ctx, planes, 3, format_bpp (src->format)));
}

int
schro_hipframe_add (SchroHipFrame * dest, SchroHipFrame * src)
{
  return add_or_subtract (dest, src, false);
}

int
schro_hipframe_subtract (SchroHipFrame * dest, SchroHipFrame * src)
{
  return add_or_subtract (dest, src, true);
}

// schro_encoder_quantise_subband (schroencoder.c:3729-3785) over every sub-band of the three components, iwt_frame and
// quant_frame on the device.  The records of a picture geometry (schro_hip_codeblock_layout) and the device summaries
// behind them (a set per queue) are the context's, rebuilt when the geometry changes; a call fills in the quant indices.
int
schro_hipframe_quantise (SchroHipFrame * quant_frame, SchroHipFrame * iwt_frame, const SchroHipParams * params,
    const int *const quant_indices[3], SchroHipCodeblockSummary * const summary[3])
{
  SCHRO_HIP_REQUIRE (quant_frame && iwt_frame && params && quant_indices && summary && frame_ctx (iwt_frame)
      && quant_frame->domain == iwt_frame->domain, "hipframe_quantise: needs two device frames of one domain, the parameters, "
      "the quant indices and the summaries");
  SchroHipContext *ctx = frame_ctx (iwt_frame);
  const int bpp = format_bpp (iwt_frame->format);
  SCHRO_HIP_REQUIRE ((bpp == 2 || bpp == 4) && quant_frame->format == iwt_frame->format && !(iwt_frame->format & 0x100),
      "hipframe_quantise: both frames must be planar s16 or s32 frames of one format");
  const int depth = params->transform_depth;
  SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "hipframe_quantise: transform_depth %d", depth);
  (void) hipSetDevice (ctx->device);
  const char *who = "hipframe_quantise";
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & c = iwt_frame->components[k], &q = quant_frame->components[k];
    const IwtSize s = iwt_size (params, k);
    SCHRO_HIP_REQUIRE (quant_indices[k] && summary[k], "hipframe_quantise: component %d has no quant indices or no summary", k);
    SCHRO_HIP_REQUIRE (holds (c, s, bpp) && q.stride == c.stride && q.height >= s.h, "hipframe_quantise: component %d: the frames "
        "(%d x %d stride %d, %d x %d stride %d) must both hold the %d x %d transform with one stride", k, c.width, c.height, c.stride,
        q.width, q.height, q.stride, s.w, s.h);
  }
  std::vector < int >key = table_key (iwt_frame, params, bpp);
  for (int l = 0; l <= depth; l++) {
    key.push_back (params->horiz_codeblocks[l]);
    key.push_back (params->vert_codeblocks[l]);
  }
  FrameQuantTable *t = ctx->frame_q_table;
  if (!t || t->key != key) {
    frame_quant_table_free (ctx);
    std::unique_ptr < FrameQuantTable > fresh (new FrameQuantTable ());
    fresh->d_summary = nullptr;
    fresh->total = 0;
    for (int k = 0; k < 3; k++) {
      SCHRO_HIP_TRY (layout_records (who, k, iwt_size (params, k), params, iwt_frame->components[k].stride, bpp, fresh->recs[k]));
      fresh->dc_first[k] = params->horiz_codeblocks[0] * params->vert_codeblocks[0];
      fresh->total += fresh->recs[k].size ();
    }
    if (hipMalloc ((void **) &fresh->d_summary, SchroHipContext::kQueues * fresh->total * sizeof (SchroHipCodeblockSummary)) != hipSuccess)
      return set_error (SCHRO_HIP_ENOMEM, "hipframe_quantise: %zu summaries", fresh->total);
    fresh->key = key;
    ctx->frame_q_table = t = fresh.release ();
  }
  const int intra = params->num_refs == 0;
  SchroHipCodeblockSummary *const d_summary = t->d_summary + (size_t) ctx->cur * t->total;       // the selected queue's
  SchroHipQuantPlane planes[3];
  size_t first = 0;
  for (int k = 0; k < 3; k++) {
    const int n = (int) t->recs[k].size ();
    SCHRO_HIP_TRY (set_quant_indices (who, k, t->recs[k], quant_indices[k]));
    const SchroHipFrameData & c = iwt_frame->components[k];
    const IwtSize s = iwt_size (params, k);
    SchroHipQuantPlane & pl = planes[k];
    memset (&pl, 0, sizeof (pl));
    pl.coeffs = c.data;
    pl.quant = quant_frame->components[k].data;
    pl.bytes = (size_t) c.stride * (size_t) s.h;
    pl.codeblocks = t->recs[k].data ();
    pl.ncodeblocks = n;
    pl.is_intra = intra;
    pl.dc_predict_first = intra ? t->dc_first[k] : 0;
    pl.dc_width = s.w >> depth;
    pl.dc_height = s.h >> depth;
    pl.summary = d_summary + first;
    first += (size_t) n;
  }
  int r = quantise_batch_run (ctx, planes, 3, bpp, true);
  first = 0;
  for (int k = 0; k < 3 && !r; k++) {
    const size_t n = t->recs[k].size ();
    if (hipMemcpyAsync (summary[k], d_summary + first, n * sizeof (SchroHipCodeblockSummary), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      r = set_error (SCHRO_HIP_EDEVICE, "hipframe_quantise: the copy of component %d's summaries failed", k);
    first += n;
  }
  return stage_done (ctx, r);
}

// schro_encoder_generate_subband_histograms (schroquantiser.c:618-637) with iwt_frame on the device.  The band records
// of a picture geometry (schro_hip_codeblock_layout with 1 x 1 codeblocks: one record per sub-band) and the counts behind
// them (on the device and in pinned host memory, a set per queue) are the context's, rebuilt when the geometry changes.
int
schro_hipframe_subband_histograms (SchroHipFrame * iwt_frame, const SchroHipParams * params, SchroHipHistogram * hists,
    uint32_t * overflow)
{
  SCHRO_HIP_REQUIRE (iwt_frame && params && hists && frame_ctx (iwt_frame),
      "hipframe_subband_histograms: needs a device frame, the parameters and the histograms");
  SchroHipContext *ctx = frame_ctx (iwt_frame);
  const int bpp = format_bpp (iwt_frame->format);
  SCHRO_HIP_REQUIRE ((bpp == 2 || bpp == 4) && !(iwt_frame->format & 0x100),
      "hipframe_subband_histograms: the frame must be a planar s16 or s32 frame");
  const int depth = params->transform_depth;
  SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "hipframe_subband_histograms: transform_depth %d", depth);
  (void) hipSetDevice (ctx->device);
  const int nb = 1 + 3 * depth;
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & c = iwt_frame->components[k];
    const IwtSize s = iwt_size (params, k);
    SCHRO_HIP_REQUIRE (holds (c, s, bpp), "hipframe_subband_histograms: component %d: the frame (%d x %d stride %d) must hold the "
        "%d x %d transform", k, c.width, c.height, c.stride, s.w, s.h);
  }
  const std::vector < int >key = table_key (iwt_frame, params, bpp);
  FrameHistTable *t = ctx->frame_h_table;
  if (!t || t->key != key) {
    frame_hist_table_free (ctx);
    t = new FrameHistTable ();
    t->d_counts = t->h_counts = nullptr;
    t->total = (size_t) 3 * nb;
    const int ones[7] = { 1, 1, 1, 1, 1, 1, 1 };
    std::vector < SchroHipCodeblock > recs (nb);
    for (int k = 0; k < 3; k++) {
      const IwtSize s = iwt_size (params, k);
      const int n = schro_hip_codeblock_layout (s.w, s.h, depth, ones, ones, iwt_frame->components[k].stride, bpp, recs.data (), nb);
      if (n != nb) {
        delete t;
        return n < 0 ? n : set_error (SCHRO_HIP_EINVAL, "hipframe_subband_histograms: component %d has %d sub-bands, not %d", k, n, nb);
      }
      t->bands[k].resize (nb);
      for (int i = 0; i < nb; i++) {
        const int level = i == 0 ? 0 : (i - 1) / 3;     // SCHRO_SUBBAND_SHIFT (position)
        SchroHipHistogramBand & b = t->bands[k][i];
        b.offset = recs[i].dst_offset;
        b.stride = recs[i].dst_stride;
        b.width = recs[i].width;
        b.height = recs[i].height;
        b.skip = 1 << std::max (0, level - 1);
        b.dc_predict = 0;
      }
    }
    const size_t bytes = SchroHipContext::kQueues * t->total * sizeof (SchroHipHistogramCounts);
    if (hipMalloc ((void **) &t->d_counts, bytes) != hipSuccess || hipHostMalloc ((void **) &t->h_counts, bytes, hipHostMallocDefault) != hipSuccess) {
      if (t->d_counts)
        (void) hipFree (t->d_counts);
      delete t;
      return set_error (SCHRO_HIP_ENOMEM, "hipframe_subband_histograms: the counts of %d sub-bands", 3 * nb);
    }
    t->key = key;
    ctx->frame_h_table = t;
  }
  SchroHipHistogramCounts *const d_counts = t->d_counts + (size_t) ctx->cur * t->total;  // the selected queue's
  SchroHipHistogramCounts *const h_counts = t->h_counts + (size_t) ctx->cur * t->total;
  SchroHipHistogramPlane planes[3];
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & c = iwt_frame->components[k];
    t->bands[k][0].dc_predict = params->num_refs == 0;
    planes[k].coeffs = c.data;
    planes[k].bytes = (size_t) c.stride * (size_t) iwt_size (params, k).h;
    planes[k].bands = t->bands[k].data ();
    planes[k].nbands = nb;
    planes[k].counts = d_counts + (size_t) k * nb;
  }
  int r = histogram_batch_run (ctx, planes, 3, bpp, true);
  if (r)
    return r;
  SCHRO_HIP_CHECK (hipMemcpyAsync (h_counts, d_counts, t->total * sizeof (SchroHipHistogramCounts), hipMemcpyDeviceToHost, ctx->stream));
  // the scale to doubles is the host's and needs the copy complete: this call waits for its queue whatever the stage setting
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < nb; i++) {
      const SchroHipHistogramBand & b = t->bands[k][i];
      const SchroHipHistogramCounts & c = h_counts[k * nb + i];
      SchroHipHistogram & out = hists[k * nb + i];
      const double skip = b.skip;
      for (int s = 0; s < SCHRO_HIP_HISTOGRAM_BINS; s++)
        out.bins[s] = c.bins[s] * skip;                 // schro_histogram_scale
      const long long rows = b.width > 0 && b.height > 0 ? (b.height + b.skip - 1) / b.skip : 0;
      out.n = (int) (rows * b.width * b.skip);
      if (overflow)
        overflow[k * nb + i] = c.overflow * (uint32_t) b.skip;
    }
  return stage_done (ctx, 0);
}

// schro_encoder_choose_quantisers for the four rate-controlled engines, synchronous: the histograms as above (their counts
// stay on the device, in the context's table for the selected queue), schro_hip_quant_choose_batch on them, the record on
// the host.  It sizes nothing itself but the device record, one per queue, the context's.
int
schro_encoder_choose_quantisers_hip (SchroHipFrame * iwt_frame, const SchroHipParams * params, const SchroHipQuantChooseSettings * settings,
    SchroHipQuantChoice * result)
{
  SCHRO_HIP_REQUIRE (iwt_frame && params && settings && result && frame_ctx (iwt_frame),
      "encoder_choose_quantisers_hip: needs a device frame, the parameters, the settings and the result");
  SchroHipContext *ctx = frame_ctx (iwt_frame);
  SCHRO_HIP_REQUIRE (ctx->qc_tables, "encoder_choose_quantisers_hip: no tables (schro_hip_quant_choose_tables comes first)");
  const int depth = params->transform_depth;
  SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "encoder_choose_quantisers_hip: transform_depth %d", depth);
  const int nb = 1 + 3 * depth;
  SchroHipQuantChoosePicture pic;
  memset (&pic, 0, sizeof (pic));
  pic.transform_depth = depth;
  pic.is_intra = params->num_refs == 0;
  pic.is_noarith = settings->is_noarith;
  pic.engine = settings->engine;
  memcpy (pic.subband_weight, settings->subband_weight, sizeof (pic.subband_weight));
  memcpy (pic.context_ratio, settings->context_ratio, sizeof (pic.context_ratio));
  pic.subband0_lambda_scale = settings->subband0_lambda_scale;
  pic.chroma_lambda_scale = settings->chroma_lambda_scale;
  pic.diagonal_lambda_scale = settings->diagonal_lambda_scale;
  pic.target = settings->target;
  (void) hipSetDevice (ctx->device);
  if (!ctx->qc_frame_choice)
    SCHRO_HIP_CHECK (hipMalloc ((void **) &ctx->qc_frame_choice, SchroHipContext::kQueues * sizeof (SchroHipQuantChoice)));
  // (the settings are the choice call's to refuse: a refusal comes after the histograms have run, before the choice is launched)
  std::vector < SchroHipHistogram > hists ((size_t) 3 * nb);
  int r = schro_hipframe_subband_histograms (iwt_frame, params, hists.data (), nullptr);
  if (r)
    return r;
  const FrameHistTable *t = ctx->frame_h_table;
  const SchroHipHistogramCounts *d_counts = t->d_counts + (size_t) ctx->cur * t->total;
  for (int k = 0; k < 3; k++)
    pic.counts[k] = d_counts + (size_t) k * nb;
  for (int i = 0; i < nb; i++)
    pic.skip[i] = t->bands[0][i].skip;
  pic.result = ctx->qc_frame_choice + ctx->cur;
  r = schro_hip_quant_choose_batch (ctx, &pic, 1);
  if (r)
    return r;
  SCHRO_HIP_CHECK (hipMemcpyAsync (result, pic.result, sizeof (SchroHipQuantChoice), hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return stage_done (ctx, 0);
}

int
schro_hipframe_shift_right (SchroHipFrame * frame, int shift)
{
  SCHRO_HIP_REQUIRE (frame && frame_ctx (frame) && !(frame->format & 0x100) && format_bpp (frame->format) > 1,
      "hipframe_shift_right: needs a device s16 / s32 frame");
  SchroHipDcPlane planes[3];
  for (int k = 0; k < 3; k++) {
    planes[k].data = frame->components[k].data;
    planes[k].stride = frame->components[k].stride;
    planes[k].width = frame->components[k].width;
    planes[k].height = frame->components[k].height;
  }
  return stage_done (frame_ctx (frame), schro_hip_shift_right_batch (frame_ctx (frame), planes, 3, format_bpp (frame->format), shift));
}

// schro_frame_downsample (dest, src) + schro_frame_mc_edgeextend (dest): one level of schro_encoder_frame_downsample
// (schroanalysis.c:24-25), the three components in one launch
int
schro_hipframe_downsample (SchroHipFrame * dest, SchroHipFrame * src)
{
  SCHRO_HIP_REQUIRE (dest && src && frame_ctx (dest) && dest->domain == src->domain, "hipframe_downsample: needs two device frames of one domain");
  SCHRO_HIP_REQUIRE (!(dest->format & 0x100) && !(src->format & 0x100) && format_bpp (dest->format) == 1 && dest->format == src->format
      && !src->is_upsampled && !dest->is_upsampled, "hipframe_downsample: needs two planar u8 frames of one chroma format");
  SCHRO_HIP_REQUIRE (dest->extension >= 0, "hipframe_downsample: negative extension %d", dest->extension);
  SchroHipDownsamplePlane planes[3];
  memset (planes, 0, sizeof (planes));
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & s = src->components[k], &d = dest->components[k];
    SCHRO_HIP_REQUIRE (s.width > 0 && s.height > 0 && d.width == (s.width + 1) / 2 && d.height == (s.height + 1) / 2,
        "hipframe_downsample: component %d is %dx%d, half of %dx%d is %dx%d", k, d.width, d.height, s.width, s.height, (s.width + 1) / 2,
        (s.height + 1) / 2);
    planes[k].src = (const uint8_t *) s.data;
    planes[k].src_stride = s.stride;
    planes[k].src_width = s.width;
    planes[k].src_height = s.height;
    planes[k].dst = (uint8_t *) d.data;
    planes[k].dst_stride = d.stride;
    planes[k].dst_extension = dest->extension;
  }
  return stage_done (frame_ctx (dest), schro_hip_downsample_batch (frame_ctx (dest), planes, 3));
}

// ---- picture statistics: the plane layer's sums, low-pass and SSIM (plane_stats.cpp) on frames.  All synchronous: each
// hands a host number back (or, the pre-filter, is the reference's plain call), whatever the stage-completion setting.

static int
stats_frame (const char *who, const SchroHipFrame * f, bool u8_only)
{
  SCHRO_HIP_REQUIRE (f && frame_ctx (f), "%s: needs a device frame", who);
  const int bpp = format_bpp (f->format);
  SCHRO_HIP_REQUIRE (!(f->format & 0x100) && !f->is_upsampled && (bpp == 1 || (bpp == 2 && !u8_only)), "%s: needs a planar %s frame", who,
      u8_only ? "u8" : "u8 or s16");
  return 0;
}

// the first `bytes` of the queue's scratch to the host, complete on return
static int
stats_fetch (SchroHipContext * ctx, void *host, size_t bytes)
{
  SCHRO_HIP_CHECK (hipMemcpyAsync (host, ctx->scratch_ref (), bytes, hipMemcpyDeviceToHost, ctx->stream));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

constexpr size_t kStatsHead = 64;       // the result words at the head of the scratch

int
schro_hipframe_calculate_average_luma (SchroHipFrame * frame, double *out)
{
  SCHRO_HIP_TRY (stats_frame ("hipframe_calculate_average_luma", frame, false));
  SCHRO_HIP_REQUIRE (out, "hipframe_calculate_average_luma: no result");
  SchroHipContext *ctx = frame_ctx (frame);
  (void) hipSetDevice (ctx->device);
  SCHRO_HIP_TRY (ensure_scratch (ctx, kStatsHead));
  const SchroHipFrameData & c = frame->components[0];
  SchroHipSumsJob job;
  memset (&job, 0, sizeof (job));
  job.a = c.data;
  job.a_stride = c.stride;
  job.bytes_per_sample = format_bpp (frame->format);
  job.width = c.width;
  job.height = c.height;
  job.result = (int64_t *) ctx->scratch_ref ();
  SCHRO_HIP_TRY (schro_hip_plane_sums_batch (ctx, &job, 1));
  int64_t words[2];
  SCHRO_HIP_TRY (stats_fetch (ctx, words, sizeof (words)));
  // schroframe.c:1652, :1678: `int sum` takes the rows' int32 sums and wraps, `int n` is the product of two ints
  const int sum = (int) (uint32_t) (uint64_t) words[0];
  const int n = (int) ((uint32_t) c.height * (uint32_t) c.width);
  *out = (double) sum / n;
  return 0;
}

int
schro_hipframe_mean_squared_error (SchroHipFrame * a, SchroHipFrame * b, double mse[3])
{
  const char *who = "hipframe_mean_squared_error";
  SCHRO_HIP_TRY (stats_frame (who, a, true));
  SCHRO_HIP_TRY (stats_frame (who, b, true));
  SCHRO_HIP_REQUIRE (mse && a->domain == b->domain, "%s: needs two frames of one domain and the result", who);
  SchroHipContext *ctx = frame_ctx (a);
  (void) hipSetDevice (ctx->device);
  SCHRO_HIP_TRY (ensure_scratch (ctx, kStatsHead));
  SchroHipSumsJob jobs[3];
  memset (jobs, 0, sizeof (jobs));
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & ca = a->components[k], &cb = b->components[k];
    // orc_sum_square_diff_u8 leaves a row's sum in an int32 (schroanalysis.c:55-60)
    SCHRO_HIP_REQUIRE (ca.width <= 33025, "%s: component %d: a row of %d samples can overflow the reference's int32 row sum", who, k, ca.width);
    jobs[k].a = ca.data;
    jobs[k].a_stride = ca.stride;
    jobs[k].bytes_per_sample = 1;
    jobs[k].width = ca.width;
    jobs[k].height = ca.height;
    jobs[k].b = (const uint8_t *) cb.data;
    jobs[k].b_stride = cb.stride;
    jobs[k].b_width = cb.width;
    jobs[k].b_height = cb.height;
    jobs[k].result = (int64_t *) ctx->scratch_ref () + 2 * k;
  }
  SCHRO_HIP_TRY (schro_hip_plane_sums_batch (ctx, jobs, 3));
  int64_t words[6];
  SCHRO_HIP_TRY (stats_fetch (ctx, words, sizeof (words)));
  for (int k = 0; k < 3; k++) {
    // the rows' sums added as doubles are exact below 2^53: the integer sum converted once is the same double
    const double n = (int) ((uint32_t) a->components[k].width * (uint32_t) a->components[k].height);       // (an int product there)
    mse[k] = (double) words[2 * k + 1] / n;
  }
  return 0;
}

int
schro_hipframe_ssim (SchroHipFrame * a, SchroHipFrame * b, double *mssim)
{
  const char *who = "hipframe_ssim";
  SCHRO_HIP_TRY (stats_frame (who, a, true));
  SCHRO_HIP_TRY (stats_frame (who, b, true));
  SCHRO_HIP_REQUIRE (mssim && a->domain == b->domain, "%s: needs two frames of one domain and the result", who);
  SchroHipContext *ctx = frame_ctx (a);
  const SchroHipFrameData & ca = a->components[0], &cb = b->components[0];
  SchroHipSsimPicture pic;
  memset (&pic, 0, sizeof (pic));
  pic.a = (const uint8_t *) ca.data;
  pic.a_stride = ca.stride;
  pic.width = ca.width;
  pic.height = ca.height;
  pic.b = (const uint8_t *) cb.data;
  pic.b_stride = cb.stride;
  pic.b_width = cb.width;
  pic.b_height = cb.height;
  pic.scratch_bytes = schro_hip_ssim_scratch_bytes (ca.width, ca.height);
  SCHRO_HIP_REQUIRE (pic.scratch_bytes, "%s: a picture of %d x %d", who, ca.width, ca.height);
  (void) hipSetDevice (ctx->device);
  SCHRO_HIP_TRY (ensure_scratch (ctx, kStatsHead + pic.scratch_bytes));
  pic.result = (SchroHipSsimResult *) ctx->scratch_ref ();
  pic.scratch = (char *) ctx->scratch_ref () + kStatsHead;
  SCHRO_HIP_TRY (schro_hip_ssim_batch (ctx, &pic, 1));
  SchroHipSsimResult res;
  SCHRO_HIP_TRY (stats_fetch (ctx, &res, sizeof (res)));
  *mssim = res.sum / (ca.width * ca.height);    // schrossim.c:124
  return 0;
}

int
schro_hipframe_filter_lowpass2 (SchroHipFrame * frame, double sigma)
{
  SCHRO_HIP_TRY (stats_frame ("hipframe_filter_lowpass2", frame, false));
  SchroHipContext *ctx = frame_ctx (frame);
  (void) hipSetDevice (ctx->device);
  SCHRO_HIP_TRY (ensure_scratch (ctx, kStatsHead));
  SCHRO_HIP_CHECK (hipMemsetAsync (ctx->scratch_ref (), 0, kStatsHead, ctx->stream));
  // schrofilter.c:790-791
  const double chroma_sigma_h = sigma / (1 << SCHRO_HIP_FORMAT_H_SHIFT (frame->format));
  const double chroma_sigma_v = sigma / (1 << SCHRO_HIP_FORMAT_V_SHIFT (frame->format));
  SchroHipLowpass2Plane planes[3];
  memset (planes, 0, sizeof (planes));
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & c = frame->components[k];
    planes[k].data = c.data;
    planes[k].stride = c.stride;
    planes[k].bytes_per_sample = format_bpp (frame->format);
    planes[k].width = c.width;
    planes[k].height = c.height;
    schro_hip_lowpass2_coeff (k ? chroma_sigma_h : sigma, planes[k].h_coeff);
    schro_hip_lowpass2_coeff (k ? chroma_sigma_v : sigma, planes[k].v_coeff);
    planes[k].out_of_range = (uint32_t *) ctx->scratch_ref () + k;
  }
  SCHRO_HIP_TRY (schro_hip_lowpass2_batch (ctx, planes, 3));
  SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  return 0;
}

int
schro_engine_get_scene_change_score_hip (SchroHipFrame * frame1, SchroHipFrame * frame2, double average_luma, double *score)
{
  SCHRO_HIP_REQUIRE (score, "engine_get_scene_change_score_hip: no result");
  // schroengine.c:327-336
  const double luma = average_luma - 16.0;
  if (luma > 0.01) {
    double mse[3];
    SCHRO_HIP_TRY (schro_hipframe_mean_squared_error (frame1, frame2, mse));
    *score = mse[0] / (luma * luma);
  } else
    *score = 1.0;
  return 0;
}

int
schro_rough_me_heirarchical_scan_nohint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame, const SchroHipParams * params, int shift,
    int distance, int ref, void *motion_vectors)
{
  SCHRO_HIP_REQUIRE (frame && ref_frame && params && motion_vectors && frame_ctx (frame) && frame->domain == ref_frame->domain,
      "rough_me_heirarchical_scan_nohint_hip: needs two device frames of one domain, the parameters and the vectors");
  SCHRO_HIP_REQUIRE (!(frame->format & 0x100) && !(ref_frame->format & 0x100) && format_bpp (frame->format) == 1
      && format_bpp (ref_frame->format) == 1 && !frame->is_upsampled && !ref_frame->is_upsampled,
      "rough_me_heirarchical_scan_nohint_hip: needs planar u8 frames");
  SCHRO_HIP_REQUIRE (frame->width == ref_frame->width && frame->height == ref_frame->height && frame->components[0].width == frame->width
      && frame->components[0].height == frame->height && ref_frame->components[0].width == frame->width
      && ref_frame->components[0].height == frame->height, "rough_me_heirarchical_scan_nohint_hip: the frames differ in size");
  // (complete on return whatever the stage-completion setting: the vectors are host memory)
  return rough_scan_nohint_run (frame_ctx (frame), (const uint8_t *) frame->components[0].data, frame->components[0].stride,
      (const uint8_t *) ref_frame->components[0].data, ref_frame->components[0].stride, frame->width, frame->height, frame->extension,
      params, shift, distance, ref, motion_vectors);
}

// the luma planes of two u8 device frames at one pyramid level, for the rough search
static int
rough_level_of (const char *who, int level, SchroHipFrame * frame, SchroHipFrame * ref_frame, SchroHipRoughPlane * out)
{
  SCHRO_HIP_REQUIRE (frame && ref_frame && frame_ctx (frame) && frame->domain == ref_frame->domain,
      "%s: level %d needs two device frames of one domain", who, level);
  SCHRO_HIP_REQUIRE (!(frame->format & 0x100) && !(ref_frame->format & 0x100) && format_bpp (frame->format) == 1
      && format_bpp (ref_frame->format) == 1 && !frame->is_upsampled && !ref_frame->is_upsampled, "%s: level %d needs planar u8 frames", who,
      level);
  SCHRO_HIP_REQUIRE (frame->width == ref_frame->width && frame->height == ref_frame->height && frame->components[0].width == frame->width
      && frame->components[0].height == frame->height && ref_frame->components[0].width == frame->width
      && ref_frame->components[0].height == frame->height, "%s: level %d: the frames differ in size", who, level);
  out->frame = (const uint8_t *) frame->components[0].data;
  out->frame_stride = frame->components[0].stride;
  out->ref = (const uint8_t *) ref_frame->components[0].data;
  out->ref_stride = ref_frame->components[0].stride;
  out->width = frame->width;
  out->height = frame->height;
  out->extension = frame->extension;
  return 0;
}

int
schro_rough_me_heirarchical_scan_hint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame, const SchroHipParams * params, int shift,
    int distance, int ref, const void *hint_motion_vectors, void *motion_vectors)
{
  const char *who = "rough_me_heirarchical_scan_hint_hip";
  SCHRO_HIP_REQUIRE (frame && ref_frame && params && hint_motion_vectors && motion_vectors,
      "%s: needs two device frames, the parameters and both vector fields", who);
  SchroHipRoughPlane level;
  int r = rough_level_of (who, shift, frame, ref_frame, &level);
  if (r)
    return r;
  // (complete on return whatever the stage-completion setting: the vectors are host memory)
  return rough_me_host_run (frame_ctx (frame), who, &level, 1, shift, params, ref, distance, distance, hint_motion_vectors, &motion_vectors);
}

int
schro_rough_me_heirarchical_scan_hip (SchroHipFrame * const *frames, SchroHipFrame * const *ref_frames, const SchroHipParams * params,
    int n_levels, int ref, void *const *motion_fields)
{
  const char *who = "rough_me_heirarchical_scan_hip";
  SCHRO_HIP_REQUIRE (frames && ref_frames && params && motion_fields, "%s: needs the frames of every level, the parameters and the fields", who);
  SCHRO_HIP_REQUIRE (n_levels >= 1 && n_levels <= SCHRO_HIP_MAX_HIER_LEVELS, "%s: %d levels, outside 1 .. %d", who, n_levels,
      SCHRO_HIP_MAX_HIER_LEVELS);
  SchroHipRoughPlane levels[SCHRO_HIP_MAX_HIER_LEVELS];
  for (int k = 1; k <= n_levels; k++) {
    int r = rough_level_of (who, k, frames[k], ref_frames[k], &levels[k - 1]);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (frames[k]->domain == frames[1]->domain, "%s: level %d is in another domain", who, k);
  }
  // schroroughmotion.c:58-60: distance 12 without a hint, 4 with one
  return rough_me_host_run (frame_ctx (frames[1]), who, levels, n_levels, 1, params, ref, 12, 4, nullptr, motion_fields + 1);
}

// the three components of two u8 device frames at one pyramid level, for the block matching
static int
hbm_level_of (const char *who, int level, SchroHipFrame * frame, SchroHipFrame * ref_frame, SchroHipHbmPlane * out)
{
  SCHRO_HIP_REQUIRE (frame && ref_frame && frame_ctx (frame) && frame->domain == ref_frame->domain,
      "%s: level %d needs two device frames of one domain", who, level);
  SCHRO_HIP_REQUIRE (!(frame->format & 0x100) && !(ref_frame->format & 0x100) && format_bpp (frame->format) == 1
      && frame->format == ref_frame->format && !frame->is_upsampled && !ref_frame->is_upsampled,
      "%s: level %d needs two planar u8 frames of one chroma format", who, level);
  const int hs = SCHRO_HIP_FORMAT_H_SHIFT (frame->format), vs = SCHRO_HIP_FORMAT_V_SHIFT (frame->format);
  for (int k = 0; k < 3; k++) {
    const SchroHipFrameData & a = frame->components[k], &b = ref_frame->components[k];
    const int cw = k ? (frame->width + (1 << hs) - 1) >> hs : frame->width, chh = k ? (frame->height + (1 << vs) - 1) >> vs : frame->height;
    SCHRO_HIP_REQUIRE (frame->width == ref_frame->width && frame->height == ref_frame->height && a.width == cw && a.height == chh
        && b.width == cw && b.height == chh, "%s: level %d: component %d of the frames is not %dx%d", who, level, k, cw, chh);
    out->frame[k] = (const uint8_t *) a.data;
    out->frame_stride[k] = a.stride;
    out->ref[k] = (const uint8_t *) b.data;
    out->ref_stride[k] = b.stride;
  }
  out->width = frame->width;
  out->height = frame->height;
  out->h_shift = hs;
  out->v_shift = vs;
  out->extension = std::min (frame->extension, ref_frame->extension);
  return 0;
}

int
schro_hierarchical_bm_scan_hint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame, const SchroHipParams * params, int shift, int h_range,
    int ref, const void *hint_motion_vectors, void *motion_vectors)
{
  const char *who = "hierarchical_bm_scan_hint_hip";
  SCHRO_HIP_REQUIRE (frame && ref_frame && params && motion_vectors, "%s: needs two device frames, the parameters and the vector field", who);
  SCHRO_HIP_REQUIRE (h_range > 0, "%s: level %d: h_range %d", who, shift, h_range);
  SchroHipHbmPlane level;
  int r = hbm_level_of (who, shift, frame, ref_frame, &level);
  if (r)
    return r;
  // (complete on return whatever the stage-completion setting: the vectors are host memory)
  return hbm_host_run (frame_ctx (frame), who, &level, 1, shift, h_range, 0, params, ref, hint_motion_vectors, &motion_vectors);
}

int
schro_hbm_scan_hip (SchroHipFrame * const *frames, SchroHipFrame * const *ref_frames, const SchroHipParams * params, int n_levels, int ref,
    int with_level0, void *const *motion_fields)
{
  const char *who = "hbm_scan_hip";
  SCHRO_HIP_REQUIRE (frames && ref_frames && params && motion_fields, "%s: needs the frames of every level, the parameters and the fields", who);
  SCHRO_HIP_REQUIRE (n_levels >= 1 && n_levels <= SCHRO_HIP_MAX_HIER_LEVELS, "%s: %d levels, outside 1 .. %d", who, n_levels,
      SCHRO_HIP_MAX_HIER_LEVELS);
  SchroHipHbmPlane levels[SCHRO_HIP_MAX_HIER_LEVELS + 1];
  memset (levels, 0, sizeof (levels));
  for (int k = n_levels; k >= (with_level0 ? 0 : 1); k--) {
    int r = hbm_level_of (who, k, frames[k], ref_frames[k], &levels[k]);
    if (r)
      return r;
    SCHRO_HIP_REQUIRE (frames[k]->domain == frames[n_levels]->domain, "%s: level %d is in another domain", who, k);
  }
  return hbm_host_run (frame_ctx (frames[n_levels]), who, levels, n_levels, 0, 0, with_level0 ? 1 : 0, params, ref, nullptr, motion_fields);
}

int
schro_encoder_motion_predict_subpel_deep_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes, const SchroHipParams * params,
    double lambda, void *const *subpel_fields)
{
  const char *who = "encoder_motion_predict_subpel_deep_hip";
  SCHRO_HIP_REQUIRE (src && ref_upframes && params && subpel_fields, "%s: needs the picture, the upsampled references, the parameters and the fields",
      who);
  SCHRO_HIP_REQUIRE (params->num_refs == 1 || params->num_refs == 2, "%s: %d references", who, params->num_refs);
  SCHRO_HIP_REQUIRE (frame_ctx (src) && !(src->format & 0x100) && format_bpp (src->format) == 1 && !src->is_upsampled
      && src->components[0].width == src->width && src->components[0].height == src->height, "%s: the picture must be a planar u8 device frame",
      who);
  SchroHipSubpelChain chains[2];
  memset (chains, 0, sizeof (chains));
  for (int r = 0; r < params->num_refs; r++) {
    const SchroHipFrame *up = ref_upframes[r];
    SCHRO_HIP_REQUIRE (up && up->is_upsampled && up->domain == src->domain && up->width == src->width && up->height == src->height
        && up->components[0].width == src->width && up->components[0].height == src->height,
        "%s: reference %d must be an upsampled device frame of the picture's size and domain", who, r);
    SCHRO_HIP_REQUIRE (subpel_fields[r], "%s: reference %d has no motion field", who, r);
    SchroHipSubpelChain & c = chains[r];
    c.src = (const uint8_t *) src->components[0].data;
    c.src_stride = src->components[0].stride;
    c.ref_up = (const uint8_t *) up->components[0].data;
    c.ref_up_stride = up->components[0].stride;
    c.width = src->width;
    c.height = src->height;
    c.extension = src->extension;
    c.x_num_blocks = params->x_num_blocks;
    c.y_num_blocks = params->y_num_blocks;
    c.xbsep_luma = params->xbsep_luma;
    c.ybsep_luma = params->ybsep_luma;
    c.mv_precision = params->mv_precision;
    c.ref_index = r;
    c.lambda = lambda;
    c.src_field = subpel_fields[r];     // (the HOST field: subpel_host_run puts both fields into the queue's scratch)
  }
  // (complete on return whatever the stage-completion setting: the fields are host memory)
  return subpel_host_run (frame_ctx (src), chains, params->num_refs);
}

// the picture of the split-2 stage from the frame layer's arguments; fields[r] are the HOST fields
static int
mode_fill_picture (const char *who, SchroHipFrame * src, SchroHipFrame * const *ref_upframes, const SchroHipParams * params, double lambda,
    const void *const *subpel_fields, SchroHipSplit2Picture & pic)
{
  SCHRO_HIP_REQUIRE (params->num_refs == 1 || params->num_refs == 2, "%s: %d references", who, params->num_refs);
  SCHRO_HIP_REQUIRE (frame_ctx (src) && !(src->format & 0x100) && format_bpp (src->format) == 1 && !src->is_upsampled
      && src->components[0].width == src->width && src->components[0].height == src->height, "%s: the picture must be a planar u8 device frame",
      who);
  memset (&pic, 0, sizeof (pic));
  pic.num_refs = params->num_refs;
  pic.width = src->width;
  pic.height = src->height;
  pic.h_shift = SCHRO_HIP_FORMAT_H_SHIFT (src->format);
  pic.v_shift = SCHRO_HIP_FORMAT_V_SHIFT (src->format);
  pic.extension = src->extension;
  pic.x_num_blocks = params->x_num_blocks;
  pic.y_num_blocks = params->y_num_blocks;
  pic.xbsep_luma = params->xbsep_luma;
  pic.ybsep_luma = params->ybsep_luma;
  pic.mv_precision = params->mv_precision;
  pic.lambda = lambda;
  for (int k = 0; k < 3; k++) {
    pic.src[k] = (const uint8_t *) src->components[k].data;
    pic.src_stride[k] = src->components[k].stride;
  }
  for (int r = 0; r < params->num_refs; r++) {
    const SchroHipFrame *up = ref_upframes[r];
    SCHRO_HIP_REQUIRE (up && up->is_upsampled && up->domain == src->domain && up->format == src->format && up->width == src->width
        && up->height == src->height, "%s: reference %d must be an upsampled device frame of the picture's format, size and domain", who, r);
    SCHRO_HIP_REQUIRE (subpel_fields[r], "%s: reference %d has no motion field", who, r);
    pic.chroma_pairs = up->is_upsampled == 2;   // (the format decides: both references have the same form)
    for (int k = 0; k < 3; k++) {
      pic.ref_up[r][k] = (const uint8_t *) up->components[k].data;
      pic.ref_up_stride[k] = up->components[k].stride;
    }
    pic.fields[r] = subpel_fields[r];   // (the HOST field: split2_host_run puts the fields into the queue's scratch)
  }
  return 0;
}

int
schro_mode_decision_split2_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes, const SchroHipParams * params, double lambda,
    const void *const *subpel_fields, void *motion, void *superblocks)
{
  const char *who = "mode_decision_split2_hip";
  SCHRO_HIP_REQUIRE (src && ref_upframes && params && subpel_fields && motion && superblocks,
      "%s: needs the picture, the upsampled references, the parameters, the fields and the two outputs", who);
  SchroHipSplit2Picture pic;
  const int r = mode_fill_picture (who, src, ref_upframes, params, lambda, subpel_fields, pic);
  if (r)
    return r;
  // (complete on return whatever the stage-completion setting: the outputs are host memory)
  return split2_host_run (frame_ctx (src), &pic, motion, superblocks);
}

int
schro_mode_decision_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes, const SchroHipParams * params, double lambda,
    const void *const *subpel_fields, const void *const *hbm_fields, void *motion, void *superblocks, void *trials, double *stats)
{
  const char *who = "mode_decision_hip";
  SCHRO_HIP_REQUIRE (src && ref_upframes && params && subpel_fields && hbm_fields && motion && superblocks && stats,
      "%s: needs the picture, the upsampled references, the parameters, the fields, the two outputs and the statistics", who);
  SchroHipModePicture pic;
  memset (&pic, 0, sizeof (pic));
  const int r = mode_fill_picture (who, src, ref_upframes, params, lambda, subpel_fields, pic.split2);
  if (r)
    return r;
  for (int k = 0; k < params->num_refs; k++)
    for (int level = 0; level < 2; level++) {
      SCHRO_HIP_REQUIRE (hbm_fields[2 * k + level], "%s: reference %d has no level-%d field", who, k, level + 1);
      pic.hbm_fields[k][level] = hbm_fields[2 * k + level];     // (HOST fields: mode_host_run puts them into the queue's scratch)
    }
  return mode_host_run (frame_ctx (src), &pic, motion, superblocks, trials, stats);
}

}                               // extern "C"
