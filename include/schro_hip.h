/*
 * schro_hip.h -- C ABI of libschro_hip.so, the MI355X (gfx950) execution
 * domain for the Dirac/VC-2 decode pixel path:
 *
 *     inverse lifting wavelet (7 filters, s16/s32)  ->  reference half-pel
 *     upsampling  ->  OBMC prediction + residual add + u8 clamp
 *
 * It occupies the slot the reference reserves for a GPU back end
 * (schroedinger/schrocuda.h:8-16, schrogpuframe.h:13-31, called from the
 * stage bodies schrodecoder.c:1697-2141), but produces the CPU path's bits:
 * every entry point is bit-exact to the reference's Orc/C implementation.
 *
 * Two layers, both plain C (pointers + sizes, no C++/torch types):
 *
 *   1. "plane" layer  -- batched kernel launches over device pointers.  This
 *      is what a host that already owns device memory binds (and what
 *      bench.py times).
 *   2. "frame" layer  -- SchroFrame-shaped structs and the stage-level calls
 *      a patched schrodecoder.c makes (INTEGRATION.md shows the patch).
 *
 * Error convention.  The reference has no return codes at this boundary:
 * device errors are SCHRO_ASSERT -> abort (schrogpuframe.c:249-253).  Here
 * every call returns 0 on success or a negative SCHRO_HIP_E* code and
 * records a message (schro_hip_last_error); schro_hip_set_abort_on_error(1)
 * restores the reference's abort behaviour.  All calls are synchronous with
 * respect to the context's stream only when they say so; the frame layer
 * returns after the work is complete, as the reference's stage scheduler
 * expects (schroasync-pthread.c:320-328).
 *
 * Threading: one SchroHipContext per exec-domain thread (the reference
 * creates exactly one such thread per GPU domain,
 * schroasync-pthread.c:362-390).  A context is not thread-safe.
 */
#ifndef SCHRO_HIP_H
#define SCHRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCHRO_HIP_OK 0
#define SCHRO_HIP_EINVAL (-1)   /* bad argument (what SCHRO_ASSERT would trap) */
#define SCHRO_HIP_EDEVICE (-2)  /* HIP runtime error */
#define SCHRO_HIP_ENOMEM (-3)
#define SCHRO_HIP_EUNSUPPORTED (-4)
#define SCHRO_HIP_ESKIPPED (-5) /* scheduler: the picture did not run, one of its references had failed */
/* r05 -- not an error of the stream but a ROUTING answer of the combine form (add = FALSE / prediction_only): this
 * picture's prediction does not fit the u8 plane it would be written to (a DC value outside [-128, 127], or picture
 * weights with a gain above 1 -- the reference's 16-bit block arithmetic wraps there, schromotion8.c:542-657), so
 * the picture takes the residual order instead (inverse transform into the residual frame, then
 * schro_motion_render_hip (..., add = TRUE, ...): INTEGRATION 3).  schro_motion_render_hip (add = FALSE) answers
 * BEFORE it launches anything when the vectors are in host memory (it scans them); with device-resident vectors the
 * launch raises a flag that the next SYNCHRONISING call of the context (a stage call with stage completion on,
 * schro_hip_synchronize, schro_hip_queue_synchronize) reports once with this code, naming the prediction_only
 * batches (schro_hip_obmc_prediction_epoch numbers them); r06: a call that only enqueues is never refused for it, and
 * schro_hip_obmc_overflowed returns every such batch's number, so a host that pipelines pictures knows exactly
 * which ones to repeat.  schro_hip_set_abort_on_error (1) never turns this code into an abort. */
#define SCHRO_HIP_ENEEDS_RESIDUAL (-6)

/* schroedinger/schrodomain.h:30-36 -- ids for the new domain */
#define SCHRO_EXEC_DOMAIN_HIP 0x0004
#define SCHRO_MEMORY_DOMAIN_HIP 0x0008

/* SchroFrameFormat bits, schroedinger/schroframe.h:16-54 */
#define SCHRO_HIP_FORMAT_DEPTH(f) ((f) & 0xc)
#define SCHRO_HIP_FORMAT_DEPTH_U8 0x00
#define SCHRO_HIP_FORMAT_DEPTH_S16 0x04
#define SCHRO_HIP_FORMAT_DEPTH_S32 0x08
#define SCHRO_HIP_FORMAT_H_SHIFT(f) ((f) & 0x1)
#define SCHRO_HIP_FORMAT_V_SHIFT(f) (((f) >> 1) & 0x1)

typedef struct SchroHipContext SchroHipContext;

/* ---- context / memory domain -------------------------------------------- */

/* replaces schro_cuda_init (schrocuda.h:8) + schro_memory_domain_new_cuda
 * (schrocuda.h:9): binds `device`, creates the stream and the size-keyed
 * device allocation cache (schrodomain.c:58-137 semantics: freed blocks are
 * kept and handed back to the next request of the same size). */
SchroHipContext *schro_hip_context_new (int device);
void schro_hip_context_free (SchroHipContext * ctx);
int schro_hip_device_count (void);
const char *schro_hip_last_error (void);
void schro_hip_set_abort_on_error (int enable);
/* schro_cuda_init (schrocuda.h:8) twin: looks at the devices (SCHRO_HIP_DEBUG prints them) */
void schro_hip_init (void);
/* The calling thread becomes the exec-domain thread of `ctx` (NULL: of none): the alloc / free table
 * of a SchroMemoryDomain carries no domain argument (schrodomain.h:18-22), so it serves the domain the
 * calling THREAD is bound to -- and fails loudly on a thread bound to none.  schro_hip_context_new
 * binds the creating thread; the scheduler's threads bind theirs. */
void schro_hip_thread_bind (SchroHipContext * ctx);
SchroHipContext *schro_hip_thread_bound (void);        /* the calling thread's domain, NULL if none */

/* SchroMemoryDomain.alloc / .free (schrodomain.h:18-22) */
void *schro_hip_domain_alloc (SchroHipContext * ctx, size_t size);
int schro_hip_domain_free (SchroHipContext * ctx, void *ptr);
/* bytes currently held by the domain (in use + cached) */
size_t schro_hip_domain_bytes (SchroHipContext * ctx);

/* host<->device copies on the context stream; *_sync wait for completion.
 * 2-D copies move `height` rows of `row_bytes`. */
int schro_hip_upload_2d (SchroHipContext * ctx, void *dst, int dst_stride,
    const void *src, int src_stride, int row_bytes, int height);
int schro_hip_download_2d (SchroHipContext * ctx, void *dst, int dst_stride,
    const void *src, int src_stride, int row_bytes, int height);
int schro_hip_memset (SchroHipContext * ctx, void *dst, int value,
    size_t bytes);
/* r03 -- asynchronous transfers (TODO-CUDA:5-7; the synchronous pattern of schrogpuframe.c:480-609).
 * Pinned host memory is what the DMA engines copy from / to at full rate without the host thread:
 * schro_hip_host_alloc for blobs, schro_memory_domain_new_hip_host () for the reference's frames
 * (schro_frame_new_and_alloc (domain, ...) then hands out pinned host frames: ordinary host memory to
 * every CPU stage).  The _async copies are enqueued on the SELECTED queue and not waited for; by
 * convention uploads go to SCHRO_HIP_QUEUE_H2D and downloads to SCHRO_HIP_QUEUE_D2H, so that picture
 * k + 1's coefficients go up and picture k - 1's pixels come down beside picture k's kernels on
 * queues 0 / 1; marks order them (upload -> mark -> the wavelet's queue waits for it; OBMC -> mark ->
 * the download queue waits for it); schro_hip_queue_synchronize waits for one queue.
 * r04 -- ORDER OF THE CALLS.  On ROCm 7.2 an asynchronous copy enqueued on a queue that waits for an event which
 * has not fired yet returns only when it has (kernels behind such a wait return at once).  A host that wants its
 * thread back enqueues a copy when everything the copy waits for has already happened: hand over picture
 * k - 2 (schro_hip_queue_mark_synchronize on ITS download mark) before enqueueing anything of picture k, and enqueue
 * the download of picture k - 1 once its kernels' mark has fired (INTEGRATION.md 3a has the loop; DESIGN.md 5 the
 * measurements: 0.2 instead of 1.4 ms of host time per step of 8 x 2160p). */
void *schro_hip_host_alloc (size_t size);
void schro_hip_host_free (void *ptr);
int schro_hip_upload_2d_async (SchroHipContext * ctx, void *dst, int dst_stride,
    const void *src, int src_stride, int row_bytes, int height);
int schro_hip_download_2d_async (SchroHipContext * ctx, void *dst, int dst_stride,
    const void *src, int src_stride, int row_bytes, int height);
int schro_hip_queue_synchronize (SchroHipContext * ctx, int queue);
/* Restricts a queue's kernels to the compute units whose bits are set in mask[0 .. words) (the queue's
 * pending work is waited for first; hipExtStreamCreateWithCUMask): two queues with disjoint masks run
 * side by side without sharing a CU's registers and LDS.
 * The queue becomes a NEW stream, and one with default flags (the runtime offers no non-blocking form of
 * this call): unlike the context's other queues it synchronises implicitly with the process's NULL stream,
 * so a synchronous hipMemcpy / hipMemset anywhere in the process serialises against it.  This library's
 * per-picture calls issue every copy, memset and kernel on an explicit queue; its set-up calls
 * (schro_hip_dequant_plan_new, a scratch buffer that grows) use synchronous ones.  If the runtime refuses the mask the
 * old queue stays in place (drained) and the call returns SCHRO_HIP_EDEVICE.  Measured slower than whole
 * batches per queue for this path: a tool for experiments, not part of the decode loop. */
int schro_hip_queue_set_cu_mask (SchroHipContext * ctx, int queue, const uint32_t * mask, int words);
/* waits for everything enqueued on both queues */
int schro_hip_synchronize (SchroHipContext * ctx);
/* the selected queue's hipStream_t, for hosts that enqueue their own work or events */
void *schro_hip_stream (SchroHipContext * ctx);

/* In-order queues per context (r03: four; 0 and 1 carry the kernels, 2 and 3 the copies).  The reference's scheduler runs the stages of different
 * pictures on several worker threads at once (schroasync-pthread.c:320-390,
 * schro_decoder_async_schedule, schrodecoder.c:1546-1682); on this domain the same
 * concurrency is two queues: the inverse wavelet is HBM-bound, OBMC is issue-bound, so
 * picture batch k's schro_hip_obmc_batch on one queue and batch k+1's schro_hip_iiwt_batch /
 * schro_hip_upsample_batch on the other run side by side.  Every call of this header goes to
 * the selected queue (0 after schro_hip_context_new); schro_hip_queue_wait makes the work
 * enqueued LATER on `waiter` start after everything enqueued SO FAR on `signaller` (the
 * render_ok / wavelet-done dependencies of schrodecoder.c:1589-1660). */
#define SCHRO_HIP_QUEUES 4
#define SCHRO_HIP_QUEUE_H2D 2      /* by convention: host-to-device copies */
#define SCHRO_HIP_QUEUE_D2H 3      /* device-to-host copies */
int schro_hip_context_select_queue (SchroHipContext * ctx, int queue);
int schro_hip_context_queue (SchroHipContext * ctx);
int schro_hip_queue_wait (SchroHipContext * ctx, int waiter, int signaller);
/* finer than "everything so far": schro_hip_queue_mark records mark m (0 .. 15) behind the work
 * enqueued so far on the SELECTED queue; schro_hip_queue_wait_mark makes the selected queue's
 * later work wait for the most recent recording of m (no-op if m was never recorded).  E.g.
 * batch k + 2's wavelet may overwrite batch k's residual frames once batch k's OBMC is done. */
#define SCHRO_HIP_MARKS 16
int schro_hip_queue_mark (SchroHipContext * ctx, int mark);
int schro_hip_queue_wait_mark (SchroHipContext * ctx, int mark);
/* the HOST waits for the latest recording of `mark` (never recorded: returns at once) */
int schro_hip_queue_mark_synchronize (SchroHipContext * ctx, int mark);

/* HIP-event timing of everything enqueued between begin and end on the
 * context stream; schro_hip_timer_end synchronises and returns milliseconds
 * (< 0 on error). */
int schro_hip_timer_begin (SchroHipContext * ctx);
float schro_hip_timer_end (SchroHipContext * ctx);

/* Per-kernel HIP-event profiling.  When enabled, every kernel launch of the
 * plane layer carries a start / stop event pair of its own (hipExtLaunchKernelGGL:
 * the kernel's begin and end as the dispatch records them, nothing extra on the
 * queue); schro_hip_profile_read synchronises and returns the summed elapsed time
 * and the number of launches of one kernel class since the last reset.  bench.py
 * uses this for the roofline figure of the dominant kernel. */
#define SCHRO_HIP_KERNEL_IIWT_FINEST 0  /* level-0 launch of the inverse wavelet */
#define SCHRO_HIP_KERNEL_IIWT_COARSE 1  /* levels >= 1 */
#define SCHRO_HIP_KERNEL_UPSAMPLE 2
#define SCHRO_HIP_KERNEL_OBMC 3
#define SCHRO_HIP_KERNEL_CONVERT 4
#define SCHRO_HIP_KERNEL_SLICES 5
#define SCHRO_HIP_KERNEL_DC_PREDICT 6
#define SCHRO_HIP_KERNEL_DEQUANT 7
#define SCHRO_HIP_KERNEL_QUANTISE 8      /* encoder: quantise_kernel */
#define SCHRO_HIP_KERNEL_QUANTISE_DC 9   /* encoder: quantise_dc_kernel (the intra LL recurrence) */
#define SCHRO_HIP_KERNEL_CLASSES 10
int schro_hip_profile_enable (SchroHipContext * ctx, int enable);
int schro_hip_profile_reset (SchroHipContext * ctx);
int schro_hip_profile_read (SchroHipContext * ctx, int kernel_class,
    double *total_ms, int *launches);

/* Which OBMC formulation a plane ran on.  schro_hip_obmc_routes copies, per
 * route, the number of planes this context's schro_hip_obmc_batch calls (and
 * so schro_motion_render_hip) have handed to launches of that route since the
 * context was created or last reset (reset != 0 clears them after the copy).
 * A (U, V) job counts two planes; a call that fails validation counts
 * nothing.  Counted on the host as the launches are enqueued: no
 * synchronisation, and profiling need not be on.  Returns 0 or an error. */
#define SCHRO_HIP_OBMC_ROUTE_ROW 0      /* obmc_row*.hip */
#define SCHRO_HIP_OBMC_ROUTE_ITEM 1     /* obmc.hip, item kernel */
#define SCHRO_HIP_OBMC_ROUTE_GENERAL 2  /* obmc.hip, per-pixel kernel */
#define SCHRO_HIP_OBMC_ROUTE_STRIP 3    /* obmc_strip.hip (experiments library only) */
#define SCHRO_HIP_OBMC_ROUTES 4
int schro_hip_obmc_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_OBMC_ROUTES], int reset);

/* Which route a picture of schro_hip_iiwt_pack_v210_batch (and so of
 * schro_frame_inverse_iwt_transform_convert_hip) took.  schro_hip_v210_routes
 * copies, per route, the number of pictures this context's calls have handed
 * to it since the context was created or last reset (reset != 0 clears them
 * after the copy).  A call that fails validation counts nothing.  Counted on
 * the host as the launches are enqueued.  Returns 0 or an error. */
#define SCHRO_HIP_V210_ROUTE_HAAR3 0    /* iiwt_haar.hip: three s32 Haar levels + v210 in one kernel */
#define SCHRO_HIP_V210_ROUTE_LEVEL 1    /* iiwt.hip: the finest level writes v210, coarser levels by the level loop */
#define SCHRO_HIP_V210_ROUTE_TWO_PASS 2 /* the pixel frame in a scratch block, then the v210 pack */
#define SCHRO_HIP_V210_ROUTES 3
int schro_hip_v210_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_V210_ROUTES], int reset);

/* The same for schro_hip_iiwt_pack_u8_batch (and so for schro_frame_inverse_iwt_transform_convert_hip /
 * _combine_convert_hip with a YUYV, UYVY or AYUV frame): pictures per route, counted on the host as the launches
 * are enqueued, nothing for a call that fails validation. */
#define SCHRO_HIP_PACK8_ROUTE_LEVEL 0   /* iiwt.hip: the finest level writes the packed rows, coarser levels by the level loop */
#define SCHRO_HIP_PACK8_ROUTE_TWO_PASS 1        /* the planar u8 picture in a scratch block, then schro_hip_pack_u8_batch's kernel */
#define SCHRO_HIP_PACK8_ROUTES 2
int schro_hip_pack8_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_PACK8_ROUTES], int reset);

/* The same for schro_hip_iiwt_pack_wide_batch (and so for schro_frame_inverse_iwt_transform_convert_hip /
 * _shift_convert_hip with a v216, ARGB or AY64 frame): pictures per route, counted on the host as the launches are
 * enqueued, nothing for a call that fails validation. */
#define SCHRO_HIP_WIDE_ROUTE_LEVEL 0    /* iiwt.hip: the finest level shifts, converts and writes the packed rows */
#define SCHRO_HIP_WIDE_ROUTE_TWO_PASS 1 /* the pixel frame in a scratch block, the shift, then schro_hip_pack_wide_batch's kernel */
#define SCHRO_HIP_WIDE_ROUTES 2
int schro_hip_wide_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_WIDE_ROUTES], int reset);

/* The same for schro_hip_unpack_iwt_batch (and so for schro_hipframe_unpack_iwt_transform): pictures per route,
 * counted on the host as the launches are enqueued, nothing for a call that fails validation. */
#define SCHRO_HIP_UNPACK_ROUTE_FUSED 0  /* iwt_fwd.hip: the level-0 launch fetches the packed rows itself */
#define SCHRO_HIP_UNPACK_ROUTE_TWO_PASS 1       /* schro_hip_unpack_batch twice through a scratch block, then schro_hip_iwt_batch */
#define SCHRO_HIP_UNPACK_ROUTES 2
int schro_hip_unpack_routes (SchroHipContext * ctx, long long counts[SCHRO_HIP_UNPACK_ROUTES], int reset);

/* ---- plane layer: batched launches --------------------------------------- */

/* One component of one picture for the inverse wavelet.
 * Replaces the level loop schro_decoder_inverse_iwt_transform
 * (schrodecoder.c:1809-1853) / schro_gpuframe_inverse_iwt_transform
 * (schrogpuframe.c:399-478).  `src` holds the coefficients in the reference's
 * in-place sub-band layout (schroparams.c:319-352: level view
 * {w>>l, h>>l, stride<<l}; even rows = [LL|HL], odd rows = [LH|HH]);
 * `dst` receives the iwt_width x iwt_height result.  src and dst must not
 * overlap (the transform is tiled, not in place); src is left untouched. */
typedef struct {
  const void *src;
  int src_stride;               /* bytes */
  void *dst;
  int dst_stride;               /* bytes */
  int width;                    /* iwt_{luma,chroma}_width  */
  int height;                   /* iwt_{luma,chroma}_height */
  /* r04 -- the combine form: the transform's last step writes the PICTURE instead of the residual frame.
   * combine 0: dst is the s16 / s32 residual plane (width x height), as above.
   * combine 1: dst is a u8 plane, out_width x out_height (the picture inside the iwt-padded transform):
   *            dst = sat_u8 (residual + pred) with the reference's 16-bit wrapping add -- the last steps of
   *            schro_motion_render (..., add = TRUE, output_frame) (orc_rrshift6_add_s16_2d / _s32_2d,
   *            schromotion8.c:852-876) --, pred (u8, out_width x out_height) = the prediction
   *            schro_hip_obmc_batch writes with prediction_only = 1.
   * combine 2: dst = sat_u8 (residual + 128): a picture without references (schro_frame_convert,
   *            orc_offsetconvert_u8_s16 / _s32, schrodecoder.c:1788-1790).
   * The residual then never exists in memory (s16, register-form filters, 8-byte aligned planes; other
   * cases go through a residual plane in the context's scratch): a step of 8 x 2160p moves 2 x 199 MB less. */
  const uint8_t *pred;
  int pred_stride;
  int out_width, out_height;
  int combine;
  /* r04 -- a picture's transform in TWO calls.  ll != NULL: the LL band of this call's COARSEST level (level
   * depth - 1: (width >> depth) x (height >> depth) samples of the plane's type) is read from this compact plane
   * instead of from the frame's LL quadrant.  The levels above 0 do not depend on the picture's prediction, so a
   * host runs them early and beside other work -- call 1: src = the frame, src_stride = 2 x the frame's stride,
   * width / 2 x height / 2 (the level-1 view of the in-place layout, schroparams.c:319-352), depth - 1 levels,
   * dst = an LL plane of the host's; call 2, once the prediction exists: the frame itself, depth 1, ll = that
   * plane, combine as above.  The two calls together are the one call, bit for bit. */
  const void *ll;
  int ll_stride;                /* bytes */
  int reserved;
} SchroHipIwtPlane;

/* depth levels, Dirac filter index 0..6 (schrobitstream.h:124-132),
 * bpp 2 (s16) or 4 (s32).  width/height must be multiples of 1<<depth.
 * Enqueues `depth` launches (coarse to fine), each covering all planes. */
int schro_hip_iiwt_batch (SchroHipContext * ctx,
    const SchroHipIwtPlane * planes, int nplanes, int depth, int filter,
    int bpp);

/* One component of one picture for the FORWARD wavelet: the level loop of schro_frame_iwt_transform /
 * schro_gpuframe_iwt_transform (schrogpuframe.h:13-31), schro_wavelet_transform_2d per level, finest level first.
 * `src` holds width x height pixels or residuals; `dst` receives the coefficients in the reference's in-place
 * sub-band layout (level view {w>>l, h>>l, stride<<l}; even rows = [LL|HL], odd rows = [LH|HH]) -- what
 * schro_hip_iiwt_batch takes as its src.  src and dst must not overlap (the transform is tiled, not in place); src is
 * left untouched, and nothing outside dst's width x height samples is written. */
typedef struct {
  const void *src;
  int src_stride;               /* bytes */
  void *dst;
  int dst_stride;               /* bytes */
  int width;                    /* iwt_{luma,chroma}_width: a multiple of 1 << depth */
  int height;                   /* iwt_{luma,chroma}_height: a multiple of 1 << depth */
} SchroHipIwtFwdPlane;

/* depth levels (1 .. 6), Dirac filter index 0..6 (schrobitstream.h:124-132), bytes_per_sample 2 (s16) or 4 (s32).
 * Enqueues `depth` launches (fine to coarse), each covering all planes; planes of unlike sizes mix freely.
 * Refused (SCHRO_HIP_EINVAL, nothing launched): a size that is not a multiple of 1 << depth, a stride shorter than
 * a row or not a multiple of the sample size, dst overlapping src, a filter, depth or sample size out of range. */
int schro_hip_iwt_batch (SchroHipContext * ctx, const SchroHipIwtFwdPlane * planes, int nplanes, int depth, int filter,
    int bytes_per_sample);

/* ---- encoder input: packed pictures to planes and to wavelet coefficients ----
 *
 * One picture of the encoder-direction schro_frame_convert (schroframe.c:869-979; schro_encoder_push_frame_full,
 * schroencoder.c:1048-1058, and the intra picture's convert into the transform frame, :2454): what the reference's chain
 * of virtual frames renders, sample for sample.
 *   source  format = SCHRO_HIP_FORMAT_YUYV / _UYVY / _AYUV / _v210 / _v216 / _AY64: the packed rows src[0] (src_stride[0]
 *           bytes apart) of a src_width x src_height picture; src_bpp and the source shifts are not read.
 *           format = 0: three planar planes of src_bpp 1 (u8) / 2 (s16) / 4 (s32) bytes per sample with the chroma shifts
 *           src_h_shift, src_v_shift (the identity unpack, schrovirtframe.c:931-932).
 *   unpack  (schrovirtframe.c:616-940) YUYV / UYVY -> u8 4:2:2, AYUV -> u8 4:4:4; v210 -> s16 4:2:2,
 *           ((word >> s) & 0x3ff) - 512, a row's last partial group as :791-858; v216 -> s16 4:2:2, the HIGH BYTE of each
 *           16-bit word and no offset (:876-888: restated, not repaired); AY64 -> s32 4:4:4, word - 32768.
 *   depth   (schroframe.c:905-924, before the chroma step) u8 -> s16 / s32: x - 128; s16 -> s32: sign extension;
 *           s32 -> s16: truncation; s16 -> u8: orc_offsetconvert_u8_s16; s32 -> u8: orc_offsetconvert_u8_s32.
 *   chroma  (schrovirtframe.c:1438-1576) u8 frames only: decimation (every second sample / row) or repetition.
 *   size    (schrovirtframe.c:1823-1960) crop or edge extension to width x height: destination sample (x, y) of a
 *           component is source sample (min (x, w_src - 1), min (y, h_src - 1)) of it, component sizes rounded up after
 *           the shifts.
 * Refused (SCHRO_HIP_EINVAL, nothing launched, the message names the picture and the reference's line): an ARGB source
 * (unpack_argb writes 16-bit samples into the lines of a frame it labels U8_444, schrovirtframe.c:693-732, 927-929);
 * AY64 -> u8 (schroframe.c:908 tests the depth of the PACKED format code, 0x107 & 0xc = S16, and reads s32 lines as
 * s16); an odd src_width for YUYV / UYVY / v216 (schrovirtframe.c:629, 881: width / 2 chroma samples of a
 * (width + 1) / 2 wide component); a chroma change on a frame that is s16 / s32 after the depth step
 * (schrovirtframe.c:1567-1569 asserts); a destination wider and shorter, or narrower and taller, than the source
 * (schrovirtframe.c:1861-1862, 1939-1940 assert); strides below a row; planar pointers or strides that are no multiple
 * of the sample size (AY64 rows: of 2); a destination plane overlapping a source of the call; sizes <= 0. */
typedef struct {
  const void *src[3];
  int src_stride[3];            /* bytes */
  int format;                   /* a packed SCHRO_HIP_FORMAT_*, or 0: planar */
  int src_width, src_height;
  int src_bpp;                  /* planar sources: 1, 2 or 4 */
  int src_h_shift, src_v_shift; /* planar sources */
  int reserved;
  void *dst[3];
  int dst_stride[3];            /* bytes */
  int dst_bpp;                  /* 1, 2 or 4 */
  int h_shift, v_shift;         /* the destination's chroma format */
  int width, height;
} SchroHipUnpackPicture;

/* One launch for all pictures of the call (at most SCHRO_HIP_UNPACK_MAX_PICTURES); pictures of unlike size, format and
 * depth mix freely.  Nothing outside the destination components' rectangles is written. */
#define SCHRO_HIP_UNPACK_MAX_PICTURES 85
int schro_hip_unpack_batch (SchroHipContext * ctx, const SchroHipUnpackPicture * pictures, int npictures);

/* One intra picture from packed bytes to wavelet coefficients.  src: the packed rows of a src_width x src_height
 * picture in `format`; width x height: the video format's picture size (the destination of the encoder's first
 * schro_frame_convert); dst[k]: the coefficient plane of component k of an iwt_width x iwt_height frame (every
 * component a multiple of 1 << depth and no smaller than the picture's), in schro_hip_iwt_batch's layout; h_shift,
 * v_shift: the transform's chroma format.  Bit for bit the chain
 *   schro_hip_unpack_batch into a width x height frame of the packed format's own depth (u8 for YUYV / UYVY / AYUV, s16
 *   for v210 / v216, s32 for AY64) and the transform's chroma format,
 *   schro_hip_unpack_batch (planar source) from that frame into an s16 / s32 frame of the transform size (the offset
 *   removed, the edges extended: schroencoder.c:2454),
 *   schro_hip_iwt_batch,
 * and refused where the chain is.  Routes, per picture and mixed freely in a call (schro_hip_unpack_routes counts them):
 *   FUSED     the level-0 launch of the forward wavelet fetches the packed rows itself (16-byte loads, the coordinate
 *             clamped to the picture: the edge extension), extracts the component and removes the offset in registers;
 *             levels 1 .. depth - 1 are schro_hip_iwt_batch's.  Needs the transform's chroma format to be the packed
 *             format's own and src, src_stride to be multiples of 16.  Taken where it did not measure slower than the
 *             chain (scripts/unpack_iwt_ab.py --sweep, profiles/unpack_iwt.txt: 8 x 2160p, depth 3):
 *               s32 coefficients  every format with every filter but Fidelity; AY64 with Fidelity too
 *               s16 coefficients  YUYV / UYVY / AYUV / v210 / v216 with Haar0 and Haar1; AY64 with every filter but Fidelity
 *   TWO_PASS  everything else: the chain above through the queue's grow-only scratch. */
typedef struct {
  const void *src;
  int src_stride;               /* bytes */
  int format;                   /* SCHRO_HIP_FORMAT_YUYV / _UYVY / _AYUV / _v210 / _v216 / _AY64 */
  int src_width, src_height;
  int width, height;            /* the picture */
  void *dst[3];
  int dst_stride[3];            /* bytes */
  int iwt_width, iwt_height;    /* the luma transform size; a chroma plane is that under the shifts, rounded up */
  int h_shift, v_shift;
  int reserved;
} SchroHipUnpackIwtPicture;

int schro_hip_unpack_iwt_batch (SchroHipContext * ctx, const SchroHipUnpackIwtPicture * pictures, int npictures, int depth,
    int filter, int bytes_per_sample);
/* The tile lengths of the two calls above, for tests and tools that place pictures around them (host only, no context):
 * values[0], values[1] = destination bytes of a row and rows of a schro_hip_unpack_batch tile; then, for wavelet filter
 * f = 0 .. 6 and coefficient size b = 0 (s16), 1 (s32), values[2 + 4 * (2 * f + b) ..] = the forward wavelet tile's useful
 * column pairs and useful row pairs (a tile writes 2 x that many samples and rows of its level) and the column pairs and
 * row pairs of halo its region reads beyond them on every side. */
#define SCHRO_HIP_UNPACK_GEOMETRY 58
void schro_hip_unpack_geometry (int values[SCHRO_HIP_UNPACK_GEOMETRY]);

/* ---- encoder analysis: the downsample pyramid and the SAD scan (schroanalysis.c:8-28, schrometric.c:31-214) ----
 *
 * One u8 component for schro_frame_downsample (schroframe.c:1449-1505): the 6, 26, 26, 6 filter down the columns,
 * rounded to u8, then along the rows, rounded again, source coordinates clamped to the picture.  dst_extension > 0 also
 * writes the apron schro_frame_mc_edgeextend (schroframe.c:1940-1997) would add -- every apron sample is computed at
 * its clamped coordinate inside the same launch, no sample another workgroup wrote is read. */
typedef struct {
  const uint8_t *src;
  int src_stride;
  int src_width, src_height;
  uint8_t *dst;                 /* pixel (0,0) of the (src_width + 1) / 2 x (src_height + 1) / 2 picture */
  int dst_stride;
  int dst_extension;            /* > 0: also write the apron of that many samples on all four sides */
} SchroHipDownsamplePlane;

/* One launch for all planes; planes of unlike sizes mix freely; a pyramid is one call per level on the same queue.
 * Nothing outside the dst picture plus its apron is written.  Refused (SCHRO_HIP_EINVAL, nothing launched):
 * non-positive sizes, a stride shorter than a row plus its aprons, dst overlapping src, a negative extension. */
int schro_hip_downsample_batch (SchroHipContext * ctx, const SchroHipDownsamplePlane * planes, int nplanes);

#define SCHRO_HIP_LIMIT_METRIC_SCAN 42  /* SCHRO_LIMIT_METRIC_SCAN, schrometric.h:16 */

/* The input members of SchroMetricScan (schrometric.h:38-53), luma only. */
typedef struct {
  int x, y, block_width, block_height;
  int ref_x, ref_y, scan_width, scan_height;    /* 1 .. SCHRO_HIP_LIMIT_METRIC_SCAN */
  int gravity_x, gravity_y;
  int dx, dy;                   /* the caller's initial vector, returned when nothing beats the gravity position */
} SchroHipMetricScan;

typedef struct {
  int dx, dy;
  uint32_t metric;
  uint32_t reserved;
} SchroHipMetricScanResult;

/* The scans of one (frame, reference) pair of u8 planes: schro_metric_scan_do_scan + schro_metric_scan_get_min of every
 * descriptor.  metrics[i * scan_height + j] = SAD (block at (x, y) of frame, block at (ref_x + i, ref_y + j) of ref); a
 * block of non-positive width or height has SAD 0.  The minimum starts at the gravity position i = gravity_x + x - ref_x,
 * j = gravity_y + y - ref_y and is replaced only by a strictly smaller metric, i outer, j inner; dx, dy change only on
 * replacement.  Samples outside a picture are its edge-extended apron: the kernel clamps coordinates.  The entries of a
 * scan's table from scan_width * scan_height on are left as they were. */
typedef struct {
  const uint8_t *frame;
  int frame_stride;
  const uint8_t *ref;
  int ref_stride;
  int width, height;            /* both planes */
  int extension;                /* the apron the reference frame WOULD have; the kernel clamps coordinates instead */
  const SchroHipMetricScan *scans;      /* HOST array, copied by the call, reusable on return */
  int nscans;
  SchroHipMetricScanResult *results;    /* device, nscans records */
  uint32_t *metrics;            /* device or NULL: scan k's table at metrics + k * 42 * 42, entry i * scan_height + j */
} SchroHipMetricScanPicture;

/* host only: schro_metric_scan_setup (schrometric.c:174-214) taken literally on scan->x, y, block_width, block_height --
 * sets ref_x, ref_y, scan_width, scan_height (which may come out <= 0: such a scan is not handed to the batch).
 * SCHRO_HIP_EINVAL where the reference asserts (dist <= 0, a window over the limit). */
int schro_hip_metric_scan_setup (SchroHipMetricScan * scan, int frame_width, int frame_height, int extension,
    int dx, int dy, int dist);
/* One launch for all scans of all pictures, one wave per scan.  Every descriptor is validated on the host first with the
 * assertions of schrometric.c:38-45; also refused: a gravity position outside the window, a window over 42, a block over
 * 64 x 64.  A refusal (SCHRO_HIP_EINVAL, nothing launched) names the picture and the scan. */
int schro_hip_metric_scan_batch (SchroHipContext * ctx, const SchroHipMetricScanPicture * pictures, int npictures);

/* ---- the hierarchical rough motion search on the device (schroroughmotion.c:47-300) ----
 *
 * A motion field on the device is a dense array of x_num_blocks * y_num_blocks SchroMotionVector records (20 bytes,
 * schromotion.h:20-37), 4-byte aligned: downloaded, it is rme->motion_fields[shift] as it is.  A call writes EVERY record
 * of every field it owns -- as schro_motion_field_set (mf, 0, 1) leaves them, then the blocks at multiples of 1 << shift --
 * and nothing outside the fields.
 *
 * One workgroup of up to SCHRO_HIP_ROUGH_WAVES waves runs one (picture, reference) chain: the blocks of a hint level
 * depend on their left, upper and upper-left neighbours, so the waves take the blocks of an anti-diagonal (i + j) / skip
 * in turn, a workgroup barrier between diagonals and between levels; fewer waves where a wave's block and window need
 * more of the workgroup's LDS (64 x 64 blocks).  No workgroup waits for another. */
#define SCHRO_HIP_ROUGH_WAVES 16
#define SCHRO_HIP_MAX_HIER_LEVELS 8     /* SCHRO_MAX_HIER_LEVELS, schromotionest.h:20 */

/* The luma planes of a frame and of its reference frame at one pyramid level. */
typedef struct {
  const uint8_t *frame;         /* device, pixel (0, 0) */
  int frame_stride;
  const uint8_t *ref;
  int ref_stride;
  int width, height;            /* both planes */
  int extension;                /* the apron the frames WOULD have (schro_metric_scan_setup); the kernel clamps coordinates */
} SchroHipRoughPlane;

/* One level of schro_rough_me_heirarchical_scan_hint (schroroughmotion.c:143-300) for one (frame, reference) pair:
 * per block (i, j) at multiples of 1 << shift the candidates -- the zero vector, the records of hint_field at
 * ((i +- skip) & mask, (j +- skip) & mask) that lie inside the field, the records of this level to the left, above and
 * above-left -- are tested with a plain SAD (:232-268: a candidate in front of the picture or ending behind it is
 * skipped, the strictly smallest metric wins, the first of equals; none left: the zero vector), then the window of
 * `distance` around the winner >> shift is scanned as schro_hip_metric_scan_batch scans (:270-295).  A block of no
 * width or height (x_num_blocks * xbsep_luma beyond the plane) has SAD 0 everywhere: its vector stays the zero vector
 * with metric 0 (the reference reads its starting minimum outside the window there); a window of no width or height
 * stores 0, 0, INT_MAX. */
typedef struct {
  const uint8_t *frame;         /* device: the planes at level `shift`, as in SchroHipRoughPlane */
  int frame_stride;
  const uint8_t *ref;
  int ref_stride;
  int width, height;
  int extension;
  int x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma;
  int shift;                    /* 1 .. 7 */
  int distance;                 /* 1 .. 20: a window of 2 * distance + 1 <= SCHRO_HIP_LIMIT_METRIC_SCAN positions */
  int ref_index;                /* 0 or 1: which of dx[], dy[] is read from the candidates and written */
  const void *hint_field;       /* device: the field of level shift + 1 (read) */
  void *field;                  /* device: the field of level `shift` (written whole) */
} SchroHipRoughHintPicture;

/* One launch, one workgroup per picture; pictures of unlike geometry, shift and ref mix.  Enqueues, does not synchronise.
 * Refused (SCHRO_HIP_EINVAL, nothing launched, the message names the picture): block counts of 0, a distance <= 0 or
 * over 20, a block over 64 x 64, ref_index outside 0 / 1, a shift outside 1 .. 7, a stride shorter than a row, a field that
 * overlaps another picture's, a plane or a hint field. */
int schro_hip_rough_hint_batch (SchroHipContext * ctx, const SchroHipRoughHintPicture * pictures, int npictures);

/* schro_rough_me_heirarchical_scan (schroroughmotion.c:47-62) for one (frame, reference) pair: the nohint level at
 * n_levels, then the hint levels n_levels - 1 .. 1, all inside ONE launch -- the fields never leave the device. */
typedef struct {
  int n_levels;                 /* 1 .. SCHRO_HIP_MAX_HIER_LEVELS; 1: only the nohint level runs */
  const SchroHipRoughPlane *levels;     /* HOST array of n_levels entries, copied by the call: levels[k] is level k + 1 */
  int x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma;
  int ref_index;                /* 0 or 1 */
  void *fields[SCHRO_HIP_MAX_HIER_LEVELS];      /* device: fields[k] is the field of level k + 1 (written whole) */
} SchroHipRoughChain;

/* One launch, one workgroup per chain.  Enqueues, does not synchronise.  The reference's distances are 12 and 4 (:58-60).
 * Refused (SCHRO_HIP_EINVAL, nothing launched, the message names the chain and the level): what
 * schro_hip_rough_hint_batch refuses, n_levels outside 1 .. 8, a plane that is not (w + 1) / 2 x (h + 1) / 2 of the
 * chain's level below it, overlapping fields. */
int schro_hip_rough_me_batch (SchroHipContext * ctx, const SchroHipRoughChain * chains, int nchains, int nohint_distance,
    int hint_distance);
/* host only: the refusals of schro_hip_rough_hint_batch / schro_hip_rough_me_batch without a context -- 0 or
 * SCHRO_HIP_EINVAL with the message the batch would give.  No pointer is dereferenced but the HOST arrays. */
int schro_hip_rough_hint_check (const SchroHipRoughHintPicture * pictures, int npictures);
int schro_hip_rough_me_check (const SchroHipRoughChain * chains, int nchains, int nohint_distance, int hint_distance);

/* ---- hierarchical block matching on the device: the DEFAULT encoder's motion search (schrohierbm.c:158-383) ----
 *
 * With enable_bigblock_estimation and enable_deep_estimation both on (the defaults, schroencoder.c:4500-4505, resolved
 * at :638-640) the encoder searches with schro_hbm_scan and schro_hierarchical_bm_scan_hint (hbm, 0, 3), not with the
 * rough search above.  Fields are laid out as above.  A call writes EVERY record of every field it owns: first as
 * schro_motion_field_set (mf, split, ref_index + 1) leaves it -- split 0 for shift > 1, 1 for shift 1, 2 for shift 0 --
 * then the blocks (i, j) at multiples of skip = 1 << shift whose origin (i * xbsep) >> shift, (j * ybsep) >> shift lies
 * inside the level's luma plane (a block off the plane keeps the first form).  Per block:
 *   * candidates, in this order: the zero vector; with a hint field, its records at (i & mask) + {0, -1, +1, 0, 0} * 2 *
 *     skip, (j & mask) + {0, 0, 0, -1, +1} * 2 * skip that lie inside the block grid, mask = ~((1 << (shift + 1)) - 1);
 *     this level's records to the left, above and above-left -- nine at the most;
 *   * duplicates: an entry goes when a LATER entry has the same dx[ref_index], dy[ref_index] (unshifted); the last entry
 *     always stays, the rest keep their order -- the order of last occurrence;
 *   * choice: per entry dx = CLAMP ((v.dx >> shift) + x0, -width0, width) - x0, dy likewise, and the SAD over the luma
 *     block AND both chroma blocks (schro_metric_block_sad_slow: chroma at x >> h_shift, (x + dx) >> h_shift, xbsep >>
 *     h_shift wide, each component clipped to what the frame's plane has left); the strictly smallest wins, the first
 *     of equals;
 *   * scan: schro_metric_scan_setup around the winner >> shift (clamped as :357-358) with h_range, over the clipped luma
 *     block, scanned as schro_hip_metric_scan_batch scans with the start vector as gravity; metric, chroma_metric 0 and
 *     dx << shift, dy << shift (int16) are stored.  dx, dy of the other reference stay 0.
 * Samples outside a plane are its edge-extended apron: the kernel clamps coordinates.  `extension` must be at least max
 * (xbsep_luma, ybsep_luma): then no candidate fails schro_frame_block_is_valid (the reference returns INT_MAX there and
 * asserts when all do, :347) and every window has a position.  The reference's frames have 32.
 * NOT covered: use_chroma (enable_chroma_me, default off) -- the scan is luma only; for 4:2:2 and 4:4:4
 * schro_metric_scan_do_scan reads uninitialised entries of its local table there (schrometric.c:84-111), so there is
 * nothing to restate and the calls have no such switch.
 *
 * One workgroup of up to SCHRO_HIP_ROUGH_WAVES waves runs one (picture, reference) chain, anti-diagonal by
 * anti-diagonal, level by level; a level without a hint field depends on its neighbours all the same.  No workgroup
 * waits for another. */

/* The three components of a frame and of its reference frame at one pyramid level. */
typedef struct {
  const uint8_t *frame[3];      /* device, pixel (0, 0) of Y, U, V */
  int frame_stride[3];
  const uint8_t *ref[3];
  int ref_stride[3];
  int width, height;            /* luma, both frames; chroma is ROUND_UP_SHIFT (width, h_shift) x ROUND_UP_SHIFT (height, v_shift) */
  int h_shift, v_shift;         /* 0, 0 (4:4:4), 1, 0 (4:2:2) or 1, 1 (4:2:0) */
  int extension;                /* the apron the frames WOULD have, >= max (xbsep_luma, ybsep_luma); the kernel clamps coordinates */
} SchroHipHbmPlane;

/* schro_hierarchical_bm_scan_hint (hbm, shift, h_range) for one (frame, reference) pair. */
typedef struct {
  SchroHipHbmPlane plane;       /* the frames at level `shift` */
  int x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma;
  int shift;                    /* 0 .. 8 */
  int h_range;                  /* 1 .. 20: a window of 2 * h_range + 1 <= SCHRO_HIP_LIMIT_METRIC_SCAN positions */
  int ref_index;                /* 0 or 1: which of dx[], dy[] is read from the candidates and written */
  const void *hint_field;       /* device: the field of level shift + 1 (read), or NULL: no parents (the top level) */
  void *field;                  /* device: the field of level `shift` (written whole) */
} SchroHipHbmLevel;

/* One launch, one workgroup per entry; entries of unlike geometry, chroma format, shift and ref mix.  Enqueues, does not
 * synchronise.  Refused (SCHRO_HIP_EINVAL, nothing launched, the message names the entry and the level): block counts
 * of 0, an h_range <= 0 or over 20, a block over 64 x 64, ref_index outside 0 / 1, a shift outside 0 .. 8, chroma shifts
 * other than the three above, a missing component, a stride shorter than a row, an extension under max (xbsep_luma,
 * ybsep_luma), a field that overlaps another entry's, a plane or a hint field. */
int schro_hip_hbm_level_batch (SchroHipContext * ctx, const SchroHipHbmLevel * levels, int nlevels);

/* schro_hbm_scan (schrohierbm.c:158-172) for one (frame, reference) pair -- levels n_levels .. 1 with h_range 20, 10, 5,
 * then MAX (3, .) -- and, with_level0, schro_hierarchical_bm_scan_hint (hbm, 0, 3) of schro_encoder_motion_predict_pel
 * (schromotionest.c:123-127) behind it, all inside ONE launch: the fields never leave the device. */
typedef struct {
  int n_levels;                 /* 1 .. SCHRO_HIP_MAX_HIER_LEVELS */
  const SchroHipHbmPlane *levels;       /* HOST array of n_levels + 1 entries, copied by the call: levels[k] is level k */
  int x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma;
  int ref_index;                /* 0 or 1 */
  void *fields[SCHRO_HIP_MAX_HIER_LEVELS + 1];  /* device: fields[k] is the field of level k (written whole) */
} SchroHipHbmChain;

/* One launch, one workgroup per chain.  Enqueues, does not synchronise.  Without with_level0, levels[0] and fields[0]
 * are not read.  Refused (SCHRO_HIP_EINVAL, nothing launched, the message names the chain and the level): what
 * schro_hip_hbm_level_batch refuses, n_levels outside 1 .. 8, a level whose chroma format differs from the chain's
 * first, a luma plane that is not (w + 1) / 2 x (h + 1) / 2 of the chain's level below it, overlapping fields. */
int schro_hip_hbm_batch (SchroHipContext * ctx, const SchroHipHbmChain * chains, int nchains, int with_level0);
/* host only: the refusals of schro_hip_hbm_level_batch / schro_hip_hbm_batch without a context -- 0 or
 * SCHRO_HIP_EINVAL with the message the batch would give.  No pointer is dereferenced but the HOST arrays. */
int schro_hip_hbm_level_check (const SchroHipHbmLevel * levels, int nlevels);
int schro_hip_hbm_check (const SchroHipHbmChain * chains, int nchains, int with_level0);

/* ---- sub-pel motion refinement on the device: schro_encoder_motion_predict_subpel_deep (schromotionest.c:246-354) ----
 *
 * The stage behind the level-0 field of the block matching above (schro_encoder_predict_subpel_picture,
 * schroencoder.c:2294-2322).  One chain is one (picture, reference) pair: the destination field is first a copy of the
 * source field; then for mvprec = 1 .. mv_precision, for every block (i, j) in raster order
 *   * a block with i * xbsep_luma >= width or j * ybsep_luma >= height is skipped, its record not even shifted;
 *   * dx[ref_index], dy[ref_index] are doubled (in int, stored back as int16) and schro_mf_vector_prediction
 *     (schromotion.c:259-312) is taken from the records to the left, above and above-left, which this pass has already
 *     doubled and refined;
 *   * min_score = estimate_sint (dx - pred_x) + estimate_sint (dy - pred_y) + lambda * metric (schropack.c:204-226);
 *   * the eight neighbours {-1,-1} {0,-1} {1,-1} {-1,0} {1,0} {-1,1} {0,1} {1,1} at x = i * (xbsep << mvprec) + dx + d.dx,
 *     y likewise, admissible iff -extension < x, (width << mvprec) + extension > x + xbsep - 1 and the same in y (the
 *     extension is not scaled, the test takes xbsep and not the clipped width): error = the SAD of the luma block clipped
 *     to MIN (xbsep, width - i * xbsep) x MIN (ybsep, height - j * ybsep) against
 *     schro_upsampled_frame_get_block_fast_precN (upframe, 0, x, y, mvprec), score = entropy of the moved vector + lambda
 *     * error; a strictly smaller score wins, the centre and earlier candidates keep ties;
 *   * a winner's offset is added, metric = its error; nothing else of the record changes.
 * `entropy + lambda * error` is a rounded product and a rounded sum as the reference's x86-64 build computes it; the
 * device code does not fuse them.
 *
 * The fetch (schroframe.c:2166-2207, 2288-2413, 2459-2482) in terms of half-pel samples S (X, Y) of the tiled image
 * above: precision 1 reads S (x + 2c, y + 2r); precision 2 is precision 3 at (2x, 2y); precision 3 has hx = x >> 2,
 * rx = x & 3 (y likewise) and gives ((4-ry)(4-rx) S (hx, hy) + (4-ry)rx S (hx+1, hy) + ry(4-rx) S (hx, hy+1) +
 * ry rx S (hx+1, hy+1) + 8) >> 4 at (+ 2c, + 2r) -- for (rx, ry) = (0, 0) the sample itself, for (2, 0) and (0, 2) the
 * reference's avgub, for the rest its orc_combine4_nxm_u8, all the same numbers.  Each tap is a RAW read of the plane
 * its parity selects; the reference's planes are edge-extended such that a raw read in the aprons is S with X clamped to
 * [0, 2 * width - 2] and Y to [0, 2 * height - 2] -- what the tiled image holds in its 32 apron columns and what the
 * kernel's row clamp gives.
 *
 * REACH.  Admissible x lie in -extension + 1 .. (width << mvprec) + extension - xbsep.  The rightmost plane column a
 * row of xbsep samples reads is
 *   precision 1:  ((2 width + e - b) >> 1) + b - 1            = width + (e + b) / 2 - 1
 *   precision 2:  ((((4 width + e - b) >> 1) + 1) >> 1) + b - 1 <= width + (e + 3 b + 2) / 4 - 1
 *   precision 3:  ((((8 width + e - b) >> 2) + 1) >> 1) + b - 1 <= width + (e + 7 b + 4) / 8 - 1
 * (e = extension, b = xbsep; the + 1 is the right tap), the leftmost (1 - e) >> mvprec >> (mvprec > 1) >= -e / 2.  With
 * b <= e all three are <= width + e - 1: inside the reference's apron of e columns; with e <= 32 they are <= width + 31:
 * inside the tiled image's.  Rows likewise.  So the calls refuse an extension under max (xbsep_luma, ybsep_luma) or over
 * 32.  (The kernel clamps the column to the image's aprons all the same.) */
typedef struct {
  const uint8_t *src;           /* device: the luma plane of the source picture, linear u8 */
  int src_stride;
  const uint8_t *ref_up;        /* device: the tiled upsampled luma image of the reference (schro_hip_upsampled_bytes), 128-byte aligned */
  int ref_up_stride;            /* bytes per band of 4 rows, as schro_hip_upsampled_bytes gives it */
  int width, height;            /* luma, both pictures */
  int extension;                /* max (xbsep_luma, ybsep_luma) .. 32: the apron the reference's frames WOULD have */
  int x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma;
  int mv_precision;             /* 0 .. 3 */
  int ref_index;                /* 0 or 1: which of dx[], dy[] is refined */
  double lambda;                /* >= 0 and finite */
  const void *src_field;        /* device: the level-0 field (read; may be `field`) */
  void *field;                  /* device: subpel_mf, x_num_blocks * y_num_blocks records */
} SchroHipSubpelChain;

/* One precision pass's errors: tables[c] (device, 4-byte aligned) receives 8 * x_num_blocks * y_num_blocks int32, eight
 * per block in candidate order -- the SAD of an admissible candidate, -1 for an inadmissible one, eight times -1 for a
 * skipped block; every entry is written.  The centre of a block is its record in chains[c].field doubled as pass mvprec
 * (1 .. chains[c].mv_precision) doubles it; the field is read, not written, src_field is not read.  One launch over the
 * blocks of all chains; chains of unlike geometry mix.  Enqueues, does not synchronise. */
int schro_hip_subpel_error_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains, int mvprec, void *const *tables);
/* One precision pass's choice from given tables (read): chains[c].field is updated in place, src_field is not read.  One
 * workgroup per chain walks the anti-diagonals of the block grid; no workgroup waits for another.  Enqueues. */
int schro_hip_subpel_choose_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains, int mvprec, void *const *tables);
/* The whole stage on the context's queue: the copy of src_field to field (where they differ), then max (mv_precision)
 * x (error, choose) with tables from the context's scratch; a chain sits out the passes beyond its own mv_precision,
 * mv_precision 0 is the copy alone.  Enqueues, does not synchronise.
 * All three refuse (SCHRO_HIP_EINVAL, nothing enqueued, the message names the chain): mv_precision outside 0 .. 3 (and a
 * pass outside 1 .. mv_precision), blocks over 32, block counts of 0, an extension outside max (xbsep_luma, ybsep_luma) ..
 * 32, (max (width, height) << mv_precision) + extension > 32767, a stride shorter than a row, an upsampled image that is
 * not 128-byte aligned or whose stride is not schro_hip_upsampled_bytes's, ref_index outside 0 / 1, a lambda that is
 * negative or not finite, NULL pointers, a field or table that overlaps anything of another chain or a picture, image
 * or table of its own (src_field == field is allowed; any other overlap of the two is not). */
int schro_hip_subpel_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains);
/* host only: the refusals of schro_hip_subpel_batch without a context.  No pointer is dereferenced but `chains`. */
int schro_hip_subpel_check (const SchroHipSubpelChain * chains, int nchains);

/* ---- mode decision on the device, the split-2 level: schro_do_split2 (schromotionest.c:1600-1807) --------------------
 *
 * The stage behind the sub-pel refinement above.  One PICTURE is a source frame with one or two references and one
 * sub-pel field per reference (field r: dx[r], dy[r] and metric are read; schro_hip_subpel_batch's output as it stands).
 * The result is SchroMotion.motion_vectors as schro_mode_decision's loop (:2616-2670) leaves it when, for every
 * superblock in raster order, it ran schro_do_split2 and then schro_motion_copy_to and nothing else: every superblock
 * split 2, every block reference 1, reference 2, both, or DC -- a field schro_hip_obmc_batch renders -- and per superblock
 * block.error, block.entropy and block.score, what a split-1 / split-0 level compares against.
 *
 * Per block (x, y), components k = 0, 1, 2 with blocks of xbsep >> shift x ybsep >> shift:
 *   0. x * xbsep_luma >= width or y * ybsep_luma >= height: the final record is best_mv = { split 2, pred_mode 1, else 0 },
 *      total_entropy += 2.  (While its superblock is worked on the reference keeps another record there, with the
 *      predicted mode and vector.  Only records of other blocks outside the picture are derived from it -- x * xbsep <
 *      width implies (x - 1) * xbsep < width, so no block inside has a neighbour outside -- and schro_motion_copy_to
 *      overwrites them all: it is not computed here.)
 *   1. per reference r: mv = field r's record with split 2, pred_mode r + 1, using_global 0 (the other bits of the flags
 *      word stay); entropy[r] = estimate_sint (dx[r] - pred_x) + estimate_sint (dy[r] - pred_y) with
 *      schro_motion_vector_prediction (schromotion.c:315-368) over the records to the left, above and above-left AS
 *      DECIDED, which skips a neighbour whose pred_mode lacks bit r (DC, and the other reference alone);
 *      schro_get_split2_metric: mv.metric == INT_MAX gives error = INT_MAX and leaves chroma_metric as copied, else
 *      chroma_metric = the SAD of the U and V blocks at (x * cb << p) + (dx[r] >> h_shift), y likewise, and error =
 *      chroma_metric + metric; score = entropy[r] + error * lambda; a strictly smaller score wins and sets best_error =
 *      metric -- LUMA ALONE.
 *   2. two references: mv (reference 2's trial) takes dx[0], dy[0] of field 0 and dx[1], dy[1] of field 1, pred_mode 3.
 *      Admissible iff for both references -extension <= X, -extension <= Y, (width << p) + extension > X + bw - 1 and the
 *      same in y, X = x * (xbsep << p) + dx[r], bw x bh the block CLIPPED to the picture, luma only.  Then metric =
 *      schro_metric_get_biref (weights 1, 1, shift 1: |orig - ((a + b + 1) >> 1)|) over luma, chroma_metric the same over U
 *      and V, score = entropy[0] + entropy[1] + (metric + chroma_metric) * lambda; a strictly smaller score wins and sets
 *      best_error = metric + chroma_metric.  Inadmissible: mv keeps reference 2's metric and chroma_metric.
 *      AT mv_precision 2 AND 3 the reference fetches the three components of a reference into ONE buffer (fd[ref],
 *      :2600-2609, filled at :1698-1737) and measures afterwards: luma is measured against V's prediction in its top-left
 *      bw[2] x bh[2] samples and U against V's prediction.  That is restated; precision 0 and 1 point into the frames.
 *   3. DC, considered iff 4 * (bw[0] * bh[0] + 2 * bw[1] * bh[1]) < best_error -- the sizes are set in step 2 only: with one
 *      reference they are 0 and the test is 0 < best_error.  The record is built IN PLACE over mv: pred_mode 0, dc[k] =
 *      schro_block_average's rounded mean - 128 over the first six bytes of the union (bytes 6-7, dy[1], stay), metric =
 *      the summed error, chroma_metric stays.  It wins iff error < best_error; its entropy is the estimate_sint of the
 *      three values, no predictor.
 *   4. total_error += best_error, total_entropy += best_entropy; per superblock error, entropy (int32, wrapping) and
 *      score = total_entropy + lambda * total_error.
 * Every product with lambda is a rounded product followed by a rounded sum, as in the sub-pel stage.
 * A block reads only the records to its left, above and above-left: any order that has those three first gives the
 * reference's result; the device walks anti-diagonals.
 *
 * The TABLE ENTRY of a block, SCHRO_HIP_SPLIT2_TABLE_INTS int32, what reads the pictures (schro_hip_split2_metric_batch):
 *   [0], [1]  chroma_metric of step 1 for reference 0, 1; -1 for a block outside the picture and for a reference the
 *             picture does not have.  (Computed whatever mv.metric is.)
 *   [2]       step 2 admissible (0 / 1); [3] its metric, [4] its chroma_metric (0 where inadmissible)
 *   [5 .. 7]  dc[0 .. 2]; [8] the summed DC error, -1 for SCHRO_METRIC_INVALID_2 (a block outside the picture)
 *   [9]       bw[0] * bh[0] + 2 * bw[1] * bh[1] of step 3 -- 0 with one reference
 *   [10 .. 15] 0
 *
 * REACH.  The luma metric of step 1 is the field's: nothing tests there whether a vector is admissible, and the chroma
 * reads go where the vector says.  With e = extension, b = xbsep_luma, p = mv_precision, a field that keeps every block
 * inside the picture plus e samples, -(e << p) <= X <= (width + e - b) << p -- what the block matching's level 0 gives
 * and the sub-pel passes (REACH above) keep -- has, for a component of shift s (xbsep a multiple of 1 << s, so x * (b >> s)
 * << p is X's origin >> s), the chroma position floor (X / 2^s): its leftmost sample column is >= -(e >> s), its
 * rightmost floor ((width + e - b) / 2^s) + (b >> s) - 1 (+ 1, the right tap, only when the position has a fraction, and
 * then the floor is one less) <= chroma width + e / 2^s - 1.  Both lie inside the reference's apron of e columns, and with
 * e <= 32 inside the tiled image's.  Rows likewise.  The bi-reference trial tests its luma reads itself.  So the calls
 * refuse an extension under max (xbsep_luma, ybsep_luma) or over 32 and a block separation that is no multiple of the
 * chroma subsampling; the kernel clamps rows and columns to the image all the same -- a field that breaks the rule reads
 * what the clamp gives, where the reference reads outside its frame.
 *
 * OUT OF SCOPE here: split 1 and split 0, schro_do_split0_biref_zero and the statistics of :2655-2681 are the stage below
 * (schro_hip_mode_decision_batch).  Out of scope of both: global motion, and a plain-plane reference for mv_precision 0:
 * the tiled image serves all four precisions, precision 0 reads S (2x, 2y). */
#define SCHRO_HIP_SPLIT2_TABLE_INTS 16
typedef struct {
  const uint8_t *src[3];        /* device: Y, U, V of the source picture, linear u8 */
  int src_stride[3];
  int num_refs;                 /* 1 or 2 */
  const uint8_t *ref_up[2][3];  /* device: per reference the tiled upsampled images of Y, U, V, 128-byte aligned */
  int ref_up_stride[3];         /* bytes per band of 4 rows, as schro_hip_upsampled_bytes gives it for the component */
  int width, height;            /* luma; a chroma component has (width + (1 << h_shift) - 1) >> h_shift columns, rows likewise */
  int h_shift, v_shift;         /* 0,0 / 1,0 / 1,1 */
  int extension;                /* max (xbsep_luma, ybsep_luma) .. 32 */
  int x_num_blocks, y_num_blocks;       /* multiples of 4 */
  int xbsep_luma, ybsep_luma;   /* multiples of 1 << h_shift, 1 << v_shift; at most 32 */
  int mv_precision;             /* 0 .. 3 */
  int chroma_pairs;             /* nonzero: ref_up[r][1] is the (U, V) pair image of an upsampled frame
                                 * (schro_hip_upsampled_pair_bytes, ref_up_stride[1] its stride), ref_up[r][2] is not read */
  double lambda;                /* >= 0 and finite */
  const void *fields[2];        /* device: the sub-pel field of each reference (read) */
  void *motion;                 /* device: x_num_blocks * y_num_blocks records of 20 bytes (written whole) */
  void *superblocks;            /* device: per superblock, raster order, int32 error, int32 entropy, double score (written whole) */
} SchroHipSplit2Picture;

/* What reads the pictures: tables[c] (device, 4-byte aligned) receives SCHRO_HIP_SPLIT2_TABLE_INTS int32 per block of
 * picture c; every entry is written.  motion and superblocks are not touched (but checked).  One launch over the
 * blocks of all pictures; pictures of unlike geometry, chroma format and num_refs mix.  Enqueues, does not synchronise. */
int schro_hip_split2_metric_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n, void *const *tables);
/* The choice from given tables and the fields (read): motion and superblocks are written.  No picture or image is read
 * (but checked).  One workgroup per picture walks the anti-diagonals of the block grid; no workgroup waits
 * for another.  Enqueues. */
int schro_hip_split2_choose_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n, void *const *tables);
/* The whole stage on the context's queue: both launches, tables from the context's scratch.  Behind
 * schro_hip_subpel_batch on the same queue it takes that call's fields without a download; schro_hip_obmc_batch behind it
 * takes `motion`.  Enqueues, does not synchronise.
 * All three refuse (SCHRO_HIP_EINVAL, nothing enqueued, the message names the picture): what the sub-pel calls refuse;
 * num_refs outside 1 / 2; chroma shifts other than 0,0 / 1,0 / 1,1; a block separation that is no multiple of the
 * subsampling; a missing component, image, field or output; block counts that are no multiples of 4; a motion field,
 * table or superblock table that overlaps anything else of the call. */
int schro_hip_split2_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n);
/* host only: the refusals of schro_hip_split2_batch without a context.  No pointer is dereferenced but `pictures`. */
int schro_hip_split2_check (const SchroHipSplit2Picture * pictures, int n);

/* ---- mode decision on the device, entire: schro_mode_decision (schromotionest.c:2587-2688) ---------------------------
 *
 * Per superblock, in raster order in the reference: schro_do_split2 (the stage above), schro_do_split1, schro_do_split0 if
 * split 1 won, schro_do_split0_biref_zero with two references, schro_block_fixup and schro_motion_copy_to of the winner,
 * and the three statistics schroencoder.c:2366-2368 reads.  A PICTURE is the split-2 stage's plus, per reference, the
 * block matching's level-1 and level-2 fields (schro_hip_hbm_batch's fields[1] and fields[2]: full grids with records
 * every 2 and every 4 blocks).  split1_mf and split0_mf of the reference are working state and no output.
 *
 * What the C text does, restated (tests/mode_ref.py is the executable form; the numbers are its rules):
 *   1. schro_do_split1 adds best_error + best_chroma_error per quadrant, and best_chroma_error stays INT_MAX unless the
 *      bi-reference trial won the quadrant.  That is signed overflow in C; the reference's build wraps, and int32
 *      two's-complement wrapping is what is restated -- AN ASSUMPTION ABOUT THE BUILD.  With s single-reference quadrants
 *      inside the picture the sum is off by s * (2^31 - 1) mod 2^32: hugely negative for odd s, the honest sum minus s for
 *      even s.  block.error, block.score, the bad-block test and mc_error all take the wrapped value.
 *   2. The hints of a split-1 quadrant and reference: its four sub-pel records, then the level-1 record, each skipped when
 *      its metric is INT_MAX or when (its vector << mv_precision) equals a listed hint's vector -- for the sub-pel records
 *      too, which are in sub-pel units already.  The level-1 hint is a COPY of the record with dx[r], dy[r] shifted; its
 *      other slot and its flag bytes travel into the winner.  Split 0: the split-1 winners of the four quadrants and
 *      reference with shift 0, then the level-2 record with shift mv_precision.
 *   3. A quadrant outside the picture keeps the predicted form at split 1: split 1, the predicted mode forced to 1 unless
 *      it is 1 or 2, the predicted vector (of reference 1) in that slot; total_entropy += 2.  Split 0 inherits the zero
 *      vector from it.
 *   4. A quadrant with no admissible hint in either reference makes the split-1 trial invalid; what the reference writes
 *      after that reaches no result, the device stops there.
 *   5. Bound tests: -extension <= X, Y and (size << p) + extension > X + bw - 1, luma, bw x bh the block CLIPPED to the
 *      picture, before any fetch of the candidate.
 *   6. The shared fetch buffers of mv_precision 2 and 3 (step 2 of the stage above) hold for the bi-reference trials of
 *      split 1, split 0 and the zero vectors, with 2x and 4x blocks.
 *   7. min_score is not updated when split 0 wins: the zero-vector trial is compared with split 1's score and can
 *      replace a split-0 winner that scores better than it.
 *   8. The split-0 trial writes only mv[0][0] of the try block; the zero-vector trial builds its record over what the
 *      earlier trials left there (bytes 1-3 and the upper flag bits stay).
 *   9. Every product with lambda is a rounded product followed by a rounded sum.
 *  10. block_size = 16 * xbsep * ybsep * 2 / 3 (integers); mc_error = sum over superblocks in raster order of
 *      (double) error * error / (double) (block_size * block_size), then / (240.0 * 240.0) / x_num_blocks * y_num_blocks / 16
 *      from left to right; badblock_ratio = #(error > 10 * block_size) / (x_num_blocks * y_num_blocks / 16);
 *      dcblock_ratio = #(pred_mode 0) / (x_num_blocks * y_num_blocks).
 *  11. A split-1 / split-0 candidate is a copy of its hint with split and pred_mode set; using_global is NOT cleared, so a
 *      hint whose bit is set has entropy 0 and carries the bit into the field.
 *  12. A superblock whose origin lies outside the picture runs into SCHRO_ASSERT (0) in the reference: refused.
 *
 * The TABLE ENTRY of a superblock, SCHRO_HIP_MODE_TABLE_INTS int32, what reads the pictures and depends on no decision
 * (schro_hip_mode_metric_batch).  Per reference r, at [264 r], 22 candidates of 12 int32: candidate 5 q + m of quadrant q
 * (0 .. 3: ii = 2 (q & 1), jj = 2 (q >> 1)) is the sub-pel record (ii + (m & 1), jj + (m >> 1)) for m < 4 and the level-1
 * record (shifted) for m = 4; candidate 20 is the level-2 record (shifted), 21 the zero vector.  Of a candidate:
 *   [0]        the split-1 bound test on its own quadrant (0 / 1); -1 for candidates 20, 21 and a quadrant outside
 *   [1]        the split-0 bound test on the superblock (0 / 1)
 *   [2 + 2 q'] the luma SAD of the vector over quadrant q', [3 + 2 q'] the chroma SAD; -1, -1 for a quadrant outside the
 *              picture and where neither [1] nor ([0] and q' its own quadrant) holds -- nothing may ask for it
 *   [10], [11] 0
 * Every int of a reference the picture does not have is -1.  A split-0 SAD is the sum over the quadrants: clipping and
 * the bilinear form are per sample.  [528 .. 531]: the zero-vector trial admissible (0 / 1), its luma and chroma metric
 * (0 where inadmissible), 0; all -1 with one reference.  The bi-reference metrics of a split-1 quadrant and of split 0
 * depend on the chosen pair and are measured inside the walk.
 *
 * REACH.  Single-reference hints of split 1 and split 0 are bound-tested on luma before anything of them is fetched: an
 * admissible hint has -e <= X and X + bw - 1 < (width << p) + e for its block clipped to the picture (e = extension, p =
 * mv_precision, X in units of 2^-p samples).  The test is the reference's own and is loose at p > 0 -- it compares units
 * with samples -- so it also admits hints whose block leaves the frame on the right; the reference then reads outside its
 * frame, here columns are clamped to the tiled image's aprons and rows to [0, 2 h - 2], as everywhere.  For the vectors
 * the block matching and the sub-pel stage produce (REACH above: every block inside the picture plus e samples; the
 * level-1 and level-2 vectors are such vectors of 2 x 2 and 4 x 4 blocks, shifted) an admissible hint's luma block of bw
 * columns lies within [-e, width + e) samples, and its chroma reads go to floor (X / 2^s) with a block of bw >> s columns:
 * leftmost column >= -(e >> s), rightmost <= floor ((width + e - bw) / 2^s) + (bw >> s) - 1 (+ 1, the right tap, only with
 * a fraction, and then the floor is one less) <= chroma width + e / 2^s - 1 -- the argument of the split-2 stage with bw
 * in place of b, which needs bw a multiple of 2^s or the block clipped at the picture's edge, where the bound is the
 * picture's.  Both lie inside the e-column apron under the same refusals: extension in max (xbsep_luma, ybsep_luma) .. 32,
 * separations multiples of the subsampling.  Rows likewise.  The bi-reference trials test their luma reads themselves. */
#define SCHRO_HIP_MODE_TABLE_INTS 532
typedef struct {
  int32_t state;                /* 1: valid, 0: tried and invalid, -1: not tried */
  int32_t error, entropy;       /* 0 unless state is 1 */
  int32_t pad;                  /* 0 */
  double score;                 /* 0 unless state is 1 */
} SchroHipModeTrial;
typedef struct {
  SchroHipSplit2Picture split2; /* everything of the split-2 stage; motion and superblocks receive the WINNER's */
  const void *hbm_fields[2][2]; /* device: per reference the block matching's level-1 and level-2 field (read) */
  void *trials;                 /* device, 8-byte aligned: per superblock four SchroHipModeTrial -- split 2, split 1, split 0,
                                 * the zero vectors (written whole) */
  void *stats;                  /* device, 8-byte aligned: three doubles -- mc_error, badblock_ratio, dcblock_ratio */
} SchroHipModePicture;

/* What reads the pictures: tables[2 c] receives the split-2 table of picture c (SCHRO_HIP_SPLIT2_TABLE_INTS int32 per
 * block, by the split-2 stage's launch), tables[2 c + 1] SCHRO_HIP_MODE_TABLE_INTS int32 per superblock; every entry is
 * written.  Two launches over all pictures.  Enqueues. */
int schro_hip_mode_metric_batch (SchroHipContext * ctx, const SchroHipModePicture * pictures, int n, void *const *tables);
/* The walk from given tables (2 n pointers as above), the fields and -- for the bi-reference trials of split 1 and
 * split 0 -- the pictures: motion, superblocks, trials and stats are written.  One workgroup per picture walks the
 * anti-diagonals of superblocks, one wave per superblock; no workgroup waits for another.  Enqueues. */
int schro_hip_mode_choose_batch (SchroHipContext * ctx, const SchroHipModePicture * pictures, int n, void *const *tables);
/* The whole stage on the context's queue, tables from the context's scratch.  Behind schro_hip_hbm_batch and
 * schro_hip_subpel_batch on the same queue it takes their fields without a download; schro_hip_obmc_batch behind it takes
 * `motion`.  Enqueues, does not synchronise.
 * All three refuse what the split-2 stage refuses, a missing level-1 / level-2 field, trial table or statistics, a grid
 * with a superblock whose origin lies outside the picture, and an output that overlaps anything else of the call. */
int schro_hip_mode_decision_batch (SchroHipContext * ctx, const SchroHipModePicture * pictures, int n);
/* host only: the refusals of schro_hip_mode_decision_batch without a context. */
int schro_hip_mode_decision_check (const SchroHipModePicture * pictures, int n);

/* intra pictures: dst_u8 = sat_u8 (src + 128), cropped to width x height;
 * replaces schro_frame_convert (ref_output_frame, frame)
 * (schrodecoder.c:1788-1790) / schro_gpuframe_convert. */
typedef struct {
  const void *src;
  int src_stride;
  uint8_t *dst;
  int dst_stride;
  int width;
  int height;
} SchroHipConvertPlane;

int schro_hip_convert_u8_batch (SchroHipContext * ctx,
    const SchroHipConvertPlane * planes, int nplanes, int bpp);

/* r06 -- dst (int16) += src (int16 when src_bytes_per_sample is 2, uint8 zero-extended when 1), 16-bit wrapping add
 * over width x height: schro_frame_add's two cases on planes (schroframe.c:1082-1135: orc_add_s16_2d,
 * orc_add_s16_u8_2d) = schro_gpuframe_add's (schrogpuframe.c:257-306).  `dst` of the plane is the int16 plane. */
int schro_hip_add_batch (SchroHipContext * ctx, const SchroHipConvertPlane * planes, int nplanes,
    int src_bytes_per_sample);

/* dst (int16) -= src (int16, or uint8 zero-extended when src_is_u8), 16-bit wrapping subtract over width x height:
 * schro_frame_subtract's two cases on planes (schroframe.c:1031-1079: orc_subtract_s16, orc_subtract_s16_u8) -- the
 * encoder's residual, picture - prediction.  The planes are schro_hip_add_batch's. */
int schro_hip_subtract_batch (SchroHipContext * ctx, const SchroHipConvertPlane * planes, int nplanes, int src_is_u8);

/* Copy-out of a decoded u8 picture into a packed output frame; replaces the
 * packed-destination case of schro_frame_convert (&output_picture, ref_output_frame)
 * in x_combine (schrodecoder.c:2011, 2052 -> schroframe.c:869-979): chroma
 * resampled by sample repetition / decimation to the packed format's chroma
 * (convert_4xx_4yy, schrovirtframe.c:1438-1537), cropped or edge-extended to
 * width x height (:1823-1895), packed (pack_yuyv / _uyvy / _ayuv :943-991,
 * 1230-1247).  On the device this halves the bytes of the device-to-host copy
 * of an 8-bit picture for a host that asked for a packed format.
 * YUYV / UYVY write width / 2 four-byte groups per row, AYUV width. */
#define SCHRO_HIP_FORMAT_YUYV 0x100     /* SCHRO_FRAME_FORMAT_YUYV, schroframe.h:36-38 */
#define SCHRO_HIP_FORMAT_UYVY 0x101
#define SCHRO_HIP_FORMAT_AYUV 0x102
#define SCHRO_HIP_FORMAT_ARGB 0x103     /* from s16 4:4:4 YCoCg-R planes */
#define SCHRO_HIP_FORMAT_v216 0x105     /* from s16 4:2:2 */
#define SCHRO_HIP_FORMAT_v210 0x106     /* 10 bit 4:2:2, six pixels in four words */
#define SCHRO_HIP_FORMAT_AY64 0x107     /* 16-bit A, Y, U, V from s32 4:4:4 */

typedef struct {
  const uint8_t *src[3];        /* Y, U, V planes (device) */
  int src_stride[3];
  int src_width, src_height;    /* luma size of the source picture */
  int src_h_shift, src_v_shift; /* its chroma subsampling (0/1) */
  uint8_t *dst;                 /* packed rows (device) */
  int dst_stride;
  int width, height;            /* size of the packed picture; not wider AND shorter (or
                                 * narrower and taller) than the source: the reference
                                 * crops both dimensions or extends both */
  int format;                   /* SCHRO_HIP_FORMAT_YUYV / _UYVY / _AYUV */
} SchroHipPackPlane;

int schro_hip_pack_u8_batch (SchroHipContext * ctx,
    const SchroHipPackPlane * planes, int nplanes);

/* The same copy-out into v210 (schroframe.c:889-891, 960-962): rows of
 * ceil (width / 6) 16-byte groups, samples beyond `width` in the last group 0.
 * src_bpp 1: u8 planes of any chroma format, 10-bit value (x << 2) | (x >> 6)
 * (pack_v210, schrovirtframe.c:1129-1210).  src_bpp 2 / 4: s16 / s32 planes --
 * the frame of a > 8-bit stream (schrodecoder.c:350-352), e.g. the 10-bit 4:2:2
 * 8K configuration -- which must be 4:2:2 as in the reference (its chroma
 * resampler only knows u8, schrovirtframe.c:1545-1575); s32 is truncated to
 * 16 bits (orc_convert_s16_s32), value clamp (x + 512, 0, 1023) (pack_v210_s16,
 * :1044-1127).  `format` of the planes is ignored; `src` / `src_stride` are in
 * bytes of the sample type. */
int schro_hip_pack_v210_batch (SchroHipContext * ctx,
    const SchroHipPackPlane * planes, int nplanes, int src_bpp);

/* r05 -- the inverse wavelet of an intra picture AND its v210 copy-out as one call (the reference's chain:
 * x_wavelet_transform, schrodecoder.c:1855-1886, then schro_frame_convert (output_picture, frame) in x_combine, :2011-2052 ->
 * schrovirtframe.c:1438-1537, :943-991).  dst receives exactly the bytes of schro_hip_iiwt_batch into a pixel frame followed by
 * schro_hip_pack_v210_batch from it.  Where the transform is the three-level s32 Haar (filters 3, 4) of a 4:2:2 picture whose
 * size is a multiple of 192 x 8 (v210 groups of 6 pixels x whole strips of the kernel; BASELINE config 5: 7680 x 4320) the copy-out is the transform kernel's epilogue and the pixel
 * frame never exists (per 8K picture 353 MB of memory traffic instead of 883 MB).  Every other picture -- any filter, depth,
 * s16 / s32, a picture smaller than its transform -- runs levels depth-1 .. 1 into a quarter-size LL plane and then one
 * launch whose finest level writes the v210 bytes (no pixel frame, no pack launch; per 8K s32 DD(9,7) picture about 520 MB
 * instead of 880 MB).  Only a dst or dst_stride that is not a multiple of 16 bytes, coefficient planes not aligned to
 * their sample size, or a dst that overlaps a coefficient plane still take the two passes.  schro_hip_v210_routes reports
 * which.  Every component must be a multiple of 2^depth in both directions (chroma: width / 2) and each src_stride must
 * hold its component's row, as schro_hip_iiwt_batch asks; a picture that is not is refused. */
typedef struct {
  const void *src[3];           /* the coefficient planes Y, U, V (device, s16 or s32), in-place sub-band layout */
  int src_stride[3];
  int width, height;            /* luma transform size (a multiple of 2^depth); chroma: >> h_shift, >> v_shift */
  int h_shift, v_shift;         /* 1, 0: v210 is a 4:2:2 format and s16 / s32 frames are not resampled (as schro_hip_pack_v210_batch) */
  uint8_t *dst;                 /* v210: 16 bytes per 6 pixels, dst_stride bytes per row */
  int dst_stride;
  int out_width, out_height;    /* the picture inside the transform's size */
} SchroHipIwtPackPicture;
int schro_hip_iiwt_pack_v210_batch (SchroHipContext * ctx, const SchroHipIwtPackPicture * pictures, int npictures, int depth,
    int filter, int bytes_per_sample);

/* The inverse wavelet of a picture, its last step -- + 128 (a picture without references) or + the u8 prediction
 * schro_hip_obmc_batch wrote with prediction_only = 1 -- and the YUYV / UYVY / AYUV copy-out as one call: x_wavelet_transform,
 * the add and schro_frame_convert (&output_picture, ...) of x_combine (schrodecoder.c:1969-2021) for a picture that is not a
 * reference, whose planar picture has no other reader.  dst receives exactly the bytes of schro_hip_iiwt_batch (combine 1 or
 * 2, the same pred: the 16-bit wrapping add and the u8 clamp described at SchroHipIwtPlane) into planar u8 planes followed by
 * schro_hip_pack_u8_batch from them: YUYV / UYVY rows of out_width / 2 four-byte groups, AYUV rows of out_width.
 * Routes, chosen per picture and mixed freely in a call (schro_hip_pack8_routes counts them):
 *   LEVEL     levels depth-1 .. 1 run into quarter-size LL planes in the queue's scratch, then ONE launch lifts the finest
 *             level of Y, U and V per tile, adds and clamps, and writes whole packed groups: no planar picture, no pack
 *             launch (about 6 bytes of memory traffic per 4:2:2 pixel with a prediction instead of 10).  Every filter and
 *             depth.  Taken when ALL of these hold:
 *               - bytes_per_sample is 2;
 *               - the filter measured faster on this route than on the two passes by more than the spread of the rounds,
 *                 with and without a prediction (8 x 2160p per call, profiles/r09_pack8_fused.txt; ms per call with a
 *                 prediction): YUYV / UYVY: filters 3, 4 (Haar: 0.163 against 0.199) and 5 (Fidelity: 0.423 against
 *                 0.719); AYUV: filters 1 (LeGall: 0.277 against 0.384), 3, 4 (0.245 against 0.382) and 5 (0.582 against
 *                 1.127).  Filters 0, 1, 2, 6 into YUYV / UYVY and 0, 2, 6 into AYUV keep the two passes, whose transform
 *                 ends in the register kernel (Daub(9,7) into YUYV: 0.304 against 0.227; DD(9,7) into AYUV: 0.294
 *                 against 0.364, a gain inside the 21 % spread of its rounds);
 *               - the source's chroma format is the packed format's own: h_shift 1, v_shift 0 for YUYV / UYVY, 0, 0 for AYUV;
 *               - dst and dst_stride are multiples of 16 bytes;
 *               - every src and src_stride is a multiple of 2 bytes;
 *               - with a prediction: every pred and pred_stride is a multiple of 8 bytes and pred_stride is at least the
 *                 component's out width rounded up to 8 (rows are read in 8-byte words, as the combine form reads them);
 *               - dst overlaps no coefficient plane and no prediction plane.
 *   TWO_PASS  everything else -- 4:2:0 sources (chroma rows repeated, schrovirtframe.c:1438-1537), a source whose chroma
 *             format is not the destination's, s32 sources, other alignments, an overlapping dst: the planar picture in
 *             the queue's scratch, then the pack kernel.
 * Refused (SCHRO_HIP_EINVAL, nothing launched or counted): what schro_hip_iiwt_batch refuses (a component that is not a
 * multiple of 2^depth, a src_stride shorter than a row), pred set for some components only, a pred_stride below the
 * component's out width, out_width x out_height outside the transform, a dst_stride below the packed row, another format,
 * bytes_per_sample other than 2 or 4. */
typedef struct {
  const void *src[3];           /* the coefficient planes Y, U, V (device, s16 or s32), in-place sub-band layout */
  int src_stride[3];
  int width, height;            /* luma transform size (a multiple of 2^depth); chroma: >> h_shift, >> v_shift */
  int h_shift, v_shift;         /* chroma format of the SOURCE picture: 0, 0 / 1, 0 / 1, 1 */
  const uint8_t *pred[3];       /* all NULL: sat_u8 (x + 128) (combine 2); all set: sat_u8 (x + pred) (combine 1); component c is
                                 * out_width x out_height, chroma rounded up after the shifts */
  int pred_stride[3];
  uint8_t *dst;                 /* packed rows */
  int dst_stride;
  int out_width, out_height;    /* the picture inside the transform's size (crop only) */
  int format;                   /* SCHRO_HIP_FORMAT_YUYV / _UYVY / _AYUV */
} SchroHipIwtPack8Picture;
int schro_hip_iiwt_pack_u8_batch (SchroHipContext * ctx, const SchroHipIwtPack8Picture * pictures, int npictures, int depth,
    int filter, int bytes_per_sample);

/* The remaining packed destinations of schro_frame_convert (schroframe.c:886-895, 957-968),
 * chosen by `format` of each plane:
 *   SCHRO_HIP_FORMAT_v216  from a 4:2:2 source brought to s16; pack_v216
 *                          (schrovirtframe.c:1007-1028) reads the s16 lines through byte
 *                          pointers and this does exactly the same: 8 bytes per pixel pair,
 *                          rows of width / 2 pairs;
 *   SCHRO_HIP_FORMAT_ARGB  from a 4:4:4 source brought to s16, YCoCg-R -> A,R,G,B bytes
 *                          (pack_argb :1265-1287), 4 bytes per pixel;
 *   SCHRO_HIP_FORMAT_AY64  from a 4:4:4 source brought to s32, 16-bit A,Y,U,V words
 *                          clamp (x + 0x8000, 0, 0xffff) (pack_ayuv64 :1302-1322), 8 bytes per pixel.
 * src_bpp 1 / 2 / 4 with the reference's depth conversions (u8: x - 128; s32 -> s16:
 * truncation; s16 -> s32: sign extension, schrovirtframe.c:1742-1817); the source's chroma
 * format must already be the destination's (the reference resamples u8 frames only). */
int schro_hip_pack_wide_batch (SchroHipContext * ctx, const SchroHipPackPlane * planes, int nplanes,
    int src_bpp);

/* The inverse wavelet of an intra picture that is not a reference, x_combine's schro_frame_shift_right (schrodecoder.c:2013-2019:
 * the stream's bit depth above the output picture's) and the v216 / ARGB / AY64 copy-out as one call -- the formats the > 8-bit
 * pictures go out in, whose frames are s32 (schrodecoder.c:350-352).  dst receives exactly the bytes of schro_hip_iiwt_batch into
 * s16 / s32 pixel planes, schro_hip_shift_right_batch on them where shift != 0, then schro_hip_pack_wide_batch from them, for
 * every input: the shift's add wraps at the sample's width, s32 is truncated to 16 bits for v216 / ARGB, s16 sign-extended
 * for AY64, and v216 reads its s16 lines through byte pointers as pack_v216 does (rows of out_width / 2 eight-byte pairs from
 * luma columns [0, out_width / 2) and chroma columns [0, out_width / 4)).
 * Routes, chosen per picture and mixed freely in a call -- formats, sizes and shifts too -- (schro_hip_wide_routes counts them):
 *   LEVEL     levels depth-1 .. 1 run into quarter-size LL planes in the queue's scratch, then ONE launch per kernel family
 *             (v216; ARGB / AY64) lifts the finest level of Y, U and V per tile, shifts, converts and writes whole 16-byte
 *             groups: no pixel frame, no shift launch, no pack launch.  Every filter, depth and sample type.  Taken when ALL
 *             of these hold:
 *               - the format x filter x sample type measured faster on this route than on the chain by more than the larger
 *                 spread of the two forms' rounds, without a shift and with one (depth 3, 8 x 2160p per call;
 *                 profiles/r10_wide_fused.txt; ms per call without a shift): every s32 combination (v216 DD(9,7) 0.226 against
 *                 0.474, ARGB 0.492 against 0.728, AY64 0.508 against 0.727), every s16 filter into v216 (DD(9,7) 0.143
 *                 against 0.250), s16 filters 0, 1, 3, 4 into ARGB (DD(9,7) 0.292 against 0.359) and 0 - 5 into AY64 (0.319
 *                 against 0.452).  s16 filters 2, 5, 6 into ARGB and 6 into AY64 keep the two passes, whose transform ends
 *                 in the register kernel (Daub(9,7) into ARGB: 0.430 against 0.401; into AY64 0.436 against 0.490, a gain
 *                 inside the 21 % spread of its rounds);
 *               - dst and dst_stride are multiples of 16 bytes;
 *               - every src and src_stride is a multiple of bytes_per_sample;
 *               - dst overlaps no coefficient plane;
 *               - a v216 row holds at least one pixel pair.
 *   TWO_PASS  everything else: the pixel planes in the queue's scratch, one shift launch per distinct non-zero shift, then the
 *             pack kernel.
 * Refused (SCHRO_HIP_EINVAL, nothing launched or counted): what schro_hip_iiwt_batch refuses (a component that is not a
 * multiple of 2^depth, a src_stride shorter than a row), a chroma format that is not the packed format's own (v216: h_shift 1,
 * v_shift 0; ARGB / AY64: 0, 0 -- as schro_hip_pack_wide_batch), out_width x out_height outside the transform, a dst_stride
 * below the packed row (v216 8 * (out_width / 2), ARGB 4 * out_width, AY64 8 * out_width), another format, shift < 0 or
 * >= 8 * bytes_per_sample, bytes_per_sample other than 2 or 4. */
typedef struct {
  const void *src[3];           /* the coefficient planes Y, U, V (device, s16 or s32), in-place sub-band layout */
  int src_stride[3];
  int width, height;            /* luma transform size (a multiple of 2^depth); chroma: >> h_shift, >> v_shift */
  int h_shift, v_shift;         /* the packed format's own chroma format: 1, 0 for v216; 0, 0 for ARGB / AY64 */
  uint8_t *dst;                 /* packed rows */
  int dst_stride;
  int out_width, out_height;    /* the picture inside the transform's size (crop only) */
  int format;                   /* SCHRO_HIP_FORMAT_v216 / _ARGB / _AY64 */
  int shift;                    /* x_combine's schro_frame_shift_right before the convert; 0: none */
} SchroHipIwtPackWidePicture;
int schro_hip_iiwt_pack_wide_batch (SchroHipContext * ctx, const SchroHipIwtPackWidePicture * pictures, int npictures, int depth,
    int filter, int bytes_per_sample);



/* ---- VC-2 low-delay transform data -----------------------------
 * Replaces schro_decoder_decode_lowdelay_transform_data (schrolowdelay.c:746-762):
 * the slices of a picture -- fixed-size and independent, offsets by the accumulator of
 * :607-631 -- are unpacked (interleaved exp-Golomb, schrounpack.c:211-241) and
 * dequantised (schro_dequantise, schroutils.c:180-189) one thread per slice straight
 * into the interleaved coefficient frame (sub-bands by schro_subband_get_frame_data,
 * schroparams.c:319-352; slice rectangles by schro_frame_data_get_codeblock,
 * schroframe.c:1865-1884), then the three LL bands are DC-predicted
 * (schro_decoder_subband_dc_predict (_s32), schrodecoder.c:3219-3277).  The host hands
 * over the compressed slice bytes (picture->lowdelay_buffer) instead of 2 or 4 bytes
 * per coefficient.
 *
 * Which arithmetic a picture gets follows the reference's own choice (:746-762):
 * bytes_per_sample 4 -> the s32 decoder; 2 with the chroma LL band divisible by the
 * slice counts -> the "fast" decoder, whose dequantisation is 16-bit throughout
 * (orc_dequantise_var_s16_ip, factor and offset truncated to int16_t, :478-479) and
 * whose slice_y_length field is sized from the short slice (:577); 2 otherwise -> the
 * "slow" decoder (int arithmetic, field sized per slice).  Where the reference is
 * undefined (a base index above 59 indexes past the fast decoder's tables; a corrupt
 * slice_y_length at the end of the buffer reads out of bounds) this library clamps the
 * quantiser index as the slow decoder does and reads guard bits. */
#define SCHRO_HIP_LIMIT_SUBBANDS 19     /* schrolimits.h */
typedef struct {
  int transform_depth;
  int iwt_luma_width, iwt_luma_height;
  int iwt_chroma_width, iwt_chroma_height;
  int n_horiz_slices, n_vert_slices;
  int slice_bytes_num, slice_bytes_denom;
  int quant_matrix[SCHRO_HIP_LIMIT_SUBBANDS];
} SchroHipLowDelayParams;

typedef struct {
  const uint8_t *slices;        /* device: the picture's slices back to back */
  size_t slices_bytes;          /* < 2^28 */
  void *comp[3];                /* device: Y, U, V coefficient planes (transform_frame) */
  int stride[3];                /* bytes */
} SchroHipLowDelayPicture;

/* the reference decoder a picture takes, from params and sample size (schrolowdelay.c:746-762) */
#define SCHRO_HIP_LOWDELAY_FAST16 0
#define SCHRO_HIP_LOWDELAY_SLOW16 1
#define SCHRO_HIP_LOWDELAY_S32 2
int schro_hip_lowdelay_arith (const SchroHipLowDelayParams * params, int bytes_per_sample);

/* all pictures share `params`; bytes_per_sample 2 (s16) or 4 (s32) */
int schro_hip_lowdelay_batch (SchroHipContext * ctx,
    const SchroHipLowDelayPicture * pictures, int npictures,
    const SchroHipLowDelayParams * params, int bytes_per_sample);

/* ---- encoder: VC-2 low-delay slices written on the device -----------------------------------
 * Replaces schro_encoder_encode_lowdelay_transform_data (schrolowdelay.c:764-1200) -- schro_encoder_pick_slice_index,
 * _estimate_slice, quantise_block, quantise_dc_block, schro_dc_predict and _encode_slice, over schro_quantise /
 * schro_dequantise (schroutils.c:179-235) and schro_pack_encode_sint / _estimate_sint (schropack.c:137-226): the bytes
 * are those the reference puts into frame->pack.  Per slice the base index is searched as the reference searches it
 * (index 0 if it fits; probes 32 .. 1 upwards; the result 1 .. 64), the sub-band indices are
 * CLAMP (base - quant_matrix[i], 0, 60) with schro_table_quant / schro_table_offset_1_2, the LL band is predicted from
 * the RECONSTRUCTED neighbours (int16_t, as the reference stores them: an LL difference at index 0 wraps), the
 * slice_y_length field is sized per slice (ilog2up (8 * slice_bytes)), the slice is padded with 1-bits.  With
 * schro_hip_iwt_batch in front this is a VC-2 low-delay intra encoder on the device.
 *
 * Two deliberate departures.  (1) The reference writes the dequantised high bands back into iwt_frame and throws the LL
 * reconstruction away (:1064-1114); this call leaves the coefficient planes untouched -- its inputs are const -- and a
 * caller that wants the reconstruction decodes the bytes with schro_hip_lowdelay_batch.  (2) Where even base index 64
 * does not fit the reference asserts (:826-830); here such a slice is cut at its last bit and counted in *overruns.
 *
 * s16 coefficients only, as the reference's encoder.  Refused (SCHRO_HIP_EINVAL, nothing enqueued, the message naming
 * the picture and member): bytes_per_sample 4 (s32 slices) or anything but 2; sizes that are not positive multiples of
 * 1 << depth; a non-positive slice_bytes_denom or slice_bytes_num below it; a chroma LL band that is not the luma LL
 * band in the frame's chroma format (the reference cuts its chroma LL rectangles from a reconstructed frame of THAT
 * size, :1164-1166, and diverges from the band where they differ); LL bands of more than 2^28 samples in the picture
 * or LL rectangles of more than 2^20 samples in one slice (the kernels index them with int); slices_bytes other than
 * slice_bytes_num * slices / slice_bytes_denom; a stride shorter than the component or odd; a NULL or odd pointer. */
typedef struct {
  const void *comp[3];          /* device: Y, U, V coefficient planes (iwt_frame), s16; not written */
  int stride[3];                /* bytes */
  uint8_t *slices;              /* device: the picture's slices back to back */
  size_t slices_bytes;          /* exactly slice_bytes_num * n_horiz_slices * n_vert_slices / slice_bytes_denom */
  uint8_t *base_index;          /* device: one byte per slice, raster order: its base index 0 .. 64 */
  uint32_t *overruns;           /* device: one word, set to the number of slices that were cut */
} SchroHipLowDelayEncodePicture;

/* all pictures share `params`; bytes_per_sample must be 2.  Three launches for the whole call */
int schro_hip_lowdelay_encode_batch (SchroHipContext * ctx,
    const SchroHipLowDelayEncodePicture * pictures, int npictures,
    const SchroHipLowDelayParams * params, int bytes_per_sample);

/* the DC prediction alone, in place on an LL band (also the intra DC prediction of the
 * core syntax, schrodecoder.c:3630-3636) */
typedef struct {
  void *data;
  int stride;
  int width, height;
} SchroHipDcPlane;
int schro_hip_dc_predict_batch (SchroHipContext * ctx,
    const SchroHipDcPlane * planes, int nplanes, int bytes_per_sample);

/* schro_frame_shift_right (schroframe.c:1265-1293) on planes, in place:
 * x = (x + ((1 << shift) >> 1)) >> shift.  The decoder applies it to an intra picture's frame
 * when the stream's bit depth exceeds the output picture's (schrodecoder.c:2013-2019). */
int schro_hip_shift_right_batch (SchroHipContext * ctx, const SchroHipDcPlane * planes, int nplanes,
    int bytes_per_sample, int shift);


/* Half-pel upsampling of one u8 component; replaces
 * schro_upsampled_frame_upsample (schroframe.c:2000-2030) /
 * schro_upsampled_gpuframe_upsample.  The device holds the reference's four planes of an
 * upsampled component -- half-pel sample (X, Y), 0 <= X < 2 * width, 0 <= Y < 2 * height, lives in
 *   plane (X & 1) + 2 * (Y & 1)   (0 integer pel, 1 h-half, 2 v-half, 3 hv-half)
 * at column X >> 1, row Y >> 1 -- in ONE buffer, tiled for the OBMC gather (r03 layout):
 *
 *   - a plane row is cut into 32-byte chunks that advance by 16 columns, so every column is
 *     stored twice and any run of up to 17 samples (one row of a block up to 16 wide, plus the
 *     X + 1 tap) starts in some chunk and ends in the same one: a lane fetches it with one
 *     byte-aligned load and needs no alignment or even / odd split instructions;
 *   - one 128-byte cache line = the same chunk of 4 consecutive rows of one plane; the four
 *     planes' lines of a (band of 4 rows, chunk) are adjacent, so the other taps of a quarter- or
 *     eighth-pel position are +-128 / +-256 bytes away and a tap the position does not use is
 *     never fetched;
 *   - 32 replicated columns in front of column 0 and behind column width - 1 (get_block clamps a
 *     block's origin to 32 pixels outside the picture, schromotion8.c:329-330), with the
 *     reference's own apron sources (schroframe.c:2012-2029: planes 0 and 1 repeat plane 0's edge
 *     sample, planes 2 and 3 plane 2's) = the half-pel column clamped to [0, 2 * width - 2]; rows
 *     have no aprons, the kernels clamp the half-pel row to [0, 2 * height - 2].
 *
 *   offset (X, Y) = (y >> 2) * stride + (xp >> 4) * 512 + plane * 128 + (y & 3) * 32 + (xp & 15)
 *   with y = Y >> 1, xp = (X >> 1) + 32; the second home of the column is 16 bytes into the chunk
 *   before: offset - 512 + 16.  stride = bytes per band of 4 rows = 512 * ((width + 79) / 16 + 1);
 *   the buffer holds ceil (height / 4) bands and must be 128-byte aligned.
 * schro_hip_upsampled_bytes () gives stride and size, schro_hip_upsampled_download () copies the
 * half-pel image to the host in linear order.  Plain (not upsampled) frames are linear.
 *
 * r04 -- PAIR images.  The U and V components of a 4:2:0 / 4:2:2 picture have the same blocks, motion
 * vectors and sample windows; a pair image holds both in the layout above over samples of TWO bytes
 * (U, V): byte column 2 * xp + c of a plane row (c = 0 U, 1 V), i.e. a chunk is 16 samples wide and
 * advances by 8, the aprons are 64 bytes:
 *   offset (X, Y, c) = (y >> 2) * stride + (xb >> 4) * 512 + plane * 128 + (y & 3) * 32 + (xb & 15),
 *   xb = 2 * ((X >> 1) + 32) + c; stride = 512 * ((2 * width + 143) / 16 + 1).
 * One load per tap then brings a block row of both components (schro_hip_obmc_batch: ref_pair).
 * schro_hip_upsample_batch writes a pair image when src_v is set (src = the U plane);
 * schro_hip_upsampled_pair_bytes / _pair_download are the helpers. */
typedef struct {
  const uint8_t *src;
  int src_stride;
  uint8_t *dst;                 /* the four tiled planes, see above */
  int dst_stride;               /* bytes per band of 4 rows, from schro_hip_upsampled_bytes / _pair_bytes */
  int width;
  int height;
  const uint8_t *src_v;         /* NULL: one component.  Else: src / src_v are the U / V planes (same size), dst a pair image */
  int src_v_stride;
} SchroHipUpsamplePlane;

/* bytes to allocate for the half-pel planes of a width x height component; *stride
 * receives the band pitch */
size_t schro_hip_upsampled_bytes (int width, int height, int *stride);
/* ... for the pair image of two width x height components */
size_t schro_hip_upsampled_pair_bytes (int width, int height, int *stride);
/* half-pel planes (on the device) -> linear host rows of 2 * width samples, 2 * height of them */
int schro_hip_upsampled_download (SchroHipContext * ctx, void *host, int host_stride,
    const void *dev, int dev_stride, int width, int height);
/* ... of a pair image: both components, each as above */
int schro_hip_upsampled_pair_download (SchroHipContext * ctx, void *host_u, void *host_v, int host_stride,
    const void *dev, int dev_stride, int width, int height);

int schro_hip_upsample_batch (SchroHipContext * ctx,
    const SchroHipUpsamplePlane * planes, int nplanes);

/* OBMC prediction + residual add + clamp for one component of one picture;
 * replaces schro_motion_render (..., add=TRUE, output_frame)
 * (schromotion.c:95 -> schro_motion_render_u8 schromotion8.c:700-929).
 *
 * mvs: DEVICE copy of the picture's SchroMotionVector array
 *      (schromotion.h:20-37, 20-byte records, x_num_blocks*y_num_blocks).
 * Block geometry is the LUMA one; the kernel derives chroma geometry from
 * chroma_h_shift/chroma_v_shift when component > 0 exactly as
 * schromotion8.c:730-758 does.
 * ref1/ref2: mv_precision == 0 -> plain u8 planes (width x height);
 *            mv_precision >= 1 -> tiled half-pel planes (see above), strides = their band pitch.
 *            ref2 may be NULL when no block uses it.
 * ref_pair:  (mv_precision >= 1, component 1 or 2) ref1 / ref2 are PAIR images of the picture's U and V
 *            components.  The U and the V plane of a picture given next to each other (U first) with the
 *            same pair images are predicted together -- one fetch per tap for both; any other use
 *            reads the component's bytes out of the pair image (correct, slower). */
typedef struct {
  const void *mvs;
  int x_num_blocks, y_num_blocks;
  int xblen_luma, yblen_luma, xbsep_luma, ybsep_luma;
  int mv_precision;
  int picture_weight_bits, picture_weight_1, picture_weight_2;
  int chroma_h_shift, chroma_v_shift;
  int component;                /* 0,1,2: selects dc[k] and chroma scaling */
  const uint8_t *ref1;
  int ref1_stride;
  const uint8_t *ref2;
  int ref2_stride;
  const void *residual;         /* s16 or s32 plane at picture coordinates */
  int residual_stride;
  int residual_bpp;             /* 2 or 4 */
  uint8_t *out;
  int out_stride;
  int width;                    /* component picture size */
  int height;
  int ref_pair;                 /* 0: one component per reference image; 1: pair images */
  int prediction_only;          /* r04: residual must be NULL; `out` receives the PREDICTION (acc + 32) >> 6 for the
                                 * combine form of schro_hip_iiwt_batch.  The prediction must fit 8 bits -- it does for
                                 * every legal stream: weights with picture_weight_1, _2 >= 0 and a sum <= 1 << bits are
                                 * required (else an error at the call), and a DC value outside [-128, 127] makes the
                                 * launch raise a flag: the next synchronising call of the context answers
                                 * SCHRO_HIP_ENEEDS_RESIDUAL and names the batch (such pictures need the
                                 * residual form, which follows the reference's 16-bit wrap-around).
                                 * r06, 2: residual NULL, `out` is an int16 plane that receives (acc - 8160) >> 6 =
                                 * the prediction - 128 in the reference's 16-bit arithmetic (orc_rrshift6_s16_ip_2d,
                                 * schroorc.orc:676-682: what schro_motion_render (add = FALSE) leaves in its dest and
                                 * schro_motion_render_cuda's contract): any weights, any DC values. */
} SchroHipObmcPlane;

int schro_hip_obmc_batch (SchroHipContext * ctx,
    const SchroHipObmcPlane * planes, int nplanes);
/* r05: prediction_only calls of schro_hip_obmc_batch are numbered per context (1, 2, ...); this is the number of
 * the latest one (0: none yet) -- what a later SCHRO_HIP_ENEEDS_RESIDUAL names. */
unsigned int schro_hip_obmc_prediction_epoch (SchroHipContext * ctx);
/* r06: the numbers of the FINISHED prediction_only batches whose predictions did not fit 8 bits and that this call has
 * not returned before, oldest first: up to `max` of them into epochs[], the count as the result (0: none; < 0: an
 * error).  Nothing is lost between calls: a batch's flag is read once its launches have completed and kept until it
 * has been returned here; a synchronising call names the same batches once in its SCHRO_HIP_ENEEDS_RESIDUAL status
 * (batches already returned here are not named again).  A host may run any number of prediction_only batches ahead:
 * the thirteenth unfinished one waits for the first. */
int schro_hip_obmc_overflowed (SchroHipContext * ctx, unsigned int *epochs, int max);

/* ---- core-syntax coefficients: dequantisation on the device ----------------
 *
 * schro_decoder_decode_subband (schrodecoder.c:3525-3640) does two things per codeblock: the
 * serial entropy decode (binary arithmetic coder or VLC), and the data-parallel rest -- zero
 * fill of zero codeblocks (:3311-3322) and dequantisation (:3072-3079, :3400-3451,
 * orc_dequantise_s16_* / _s32_ip_2d schroorc.orc:1098-1219).  The arithmetic decoder's
 * contexts look only at whether neighbouring / parent coefficients are zero and at a
 * neighbour's sign, which quantised values answer as well as dequantised ones (a non-zero value
 * stays non-zero: quant_factor >= 4), so a host decoder can keep the QUANTISED values, hand
 * them over for the non-zero codeblocks only -- 1, 2 or 4 bytes each -- and leave the dense
 * coefficient frame to the device: schro_hip_dequant_batch, then schro_hip_dc_predict_batch on
 * the LL bands of intra pictures (schrodecoder.c:3629-3636), then schro_hip_iiwt_batch. */
typedef struct {
  int dst_offset;               /* bytes from the plane's base to the codeblock's first sample */
  int dst_stride;               /* bytes between its rows: the frame stride << the sub-band's level shift
                                 * (schro_subband_get_frame_data, schroparams.c:319-368) */
  int width, height;            /* samples: xmax - xmin, ymax - ymin */
  int src_offset;               /* bytes from `values` to its quantised values, row-major and
                                 * tight; < 0: zero codeblock (nothing stored) */
  unsigned char src_bytes;      /* 1, 2 or 4 bytes per stored value (signed) */
  unsigned char quant_index;    /* ctx->quant_index of the codeblock, 0 .. 60 */
  unsigned char pad[2];
} SchroHipCodeblock;

typedef struct {
  void *dst;                    /* the component's coefficient plane (device, s16 or s32) */
  const void *values;           /* packed quantised values of its non-zero codeblocks (device) */
  const SchroHipCodeblock *codeblocks;  /* HOST array: every codeblock of every sub-band */
  int ncodeblocks;
  int is_intra;                 /* params->num_refs == 0: schro_table_offset_1_2, else _3_8 */
} SchroHipDequantPlane;

/* arith 0: C int arithmetic (arithmetic-coded codeblocks; s32 frames); 1: the 16-bit Orc
 * arithmetic of the VLC (is_noarith) path on s16 frames.  The two differ only where 16-bit
 * products wrap, which no legal stream reaches. */
int schro_hip_dequant_batch (SchroHipContext * ctx, const SchroHipDequantPlane * planes, int nplanes,
    int bytes_per_sample, int arith);

/* r04 -- plans: the host cost of a repeated picture geometry is O (planes), not O (codeblocks).  A plan holds
 * what is fixed per picture GEOMETRY -- every record's dst_offset / dst_stride / width / height and with them the
 * launch's tiles -- on the device; a run uploads the records as they are (the device reads src_offset, src_bytes
 * and quant_index itself) and one line per plane (dst, values, is_intra).  `planes` of a run: the same planes in
 * the same order, with this batch's pointers and records; the records' geometry must be the plan's.  Results
 * are schro_hip_dequant_batch's, bit for bit.  (r03: the batch call rebuilt 15 k job records per 8 x 2160p, 1.3 of
 * the 2.3 ms of a PCIe-inclusive step with the quantised hand-over.) */
typedef struct SchroHipDequantPlan SchroHipDequantPlan;
SchroHipDequantPlan *schro_hip_dequant_plan_new (SchroHipContext * ctx, const SchroHipDequantPlane * planes, int nplanes,
    int bytes_per_sample, int arith);
int schro_hip_dequant_plan_run (SchroHipDequantPlan * plan, const SchroHipDequantPlane * planes, int nplanes);
void schro_hip_dequant_plan_free (SchroHipDequantPlan * plan);

/* The geometry of every codeblock record of one component, in the decoder's order -- sub-band index
 * 0 .. 3 * depth, in each its rows of codeblocks (schro_decoder_decode_subband, schrodecoder.c:3558-3577;
 * counts per sub-band from params->horiz_codeblocks / vert_codeblocks [0 .. depth] as
 * schro_decoder_setup_codeblocks picks them, :3280-3293; rectangles by schro_subband_get_frame_data,
 * schroparams.c:319-352): dst_offset, dst_stride, width, height filled, src_offset -1 (zero codeblock).
 * A host decoder builds the table once per picture geometry and fills src_offset / src_bytes /
 * quant_index as it entropy-decodes.  Returns the number of records (write stops at `max`). */
int schro_hip_codeblock_layout (int iwt_width, int iwt_height, int transform_depth, const int *horiz_codeblocks,
    const int *vert_codeblocks, int stride, int bytes_per_sample, SchroHipCodeblock * out, int max);

/* ---- encoder: quantisation on the device ---------------------------------------------------
 *
 * schro_encoder_quantise_subband (schroencoder.c:3729-3785) per codeblock: the quantised value goes to the quant
 * frame, and IN THE SAME PASS the dequantised value replaces the coefficient -- the reconstruction the encoder's local
 * decode runs the inverse transform on (:2697-2700).  The arithmetic is the reference's, bit for bit:
 *   s16 frames (schro_frame_data_quantise, :3485-3553): four 16-bit Orc programs by quant index -- 0: copy, the
 *     coefficients stay; a multiple of 4: orc_quantdequant2_s16 (a shift); 3: orc_quantdequant3_s16; any other:
 *     orc_quantdequant1_s16 (mulhuw by schro_table_inverse_quant, quant_offset-- above index 8).  Every step wraps at 16
 *     bits, and the reciprocal multiply is NOT schro_quantise's division (they part as early as |x| = 47).
 *   s32 frames: schro_quantise_s32 (schroutils.c:248-257), C int arithmetic with a truncating division; |x| < 2^28.
 *   offsets: schro_table_offset_1_2 when is_intra, else schro_table_offset_3_8.
 *   the LL band of an intra picture (dc_predict_first): schro_frame_data_quantise_dc_predict (:3591-3667) -- each
 *     sample is predicted from its RECONSTRUCTED left, upper and upper-left neighbours (schro_divide3 on s16,
 *     schro_divide (., 3) on s32), the difference goes through C schro_quantise / schro_dequantise, the s16 stores
 *     truncate.  A codeblock never reads its right neighbour, so the band is one raster-order recurrence in which every
 *     sample takes its own codeblock's quant index; the device sweeps its anti-diagonals.
 * One departure, deliberate: the reference's zero test on s16 (schro_frame_data_is_zero, :4043-4070) sums |q| per row in
 * 16 bits and calls a row zero when the sum is a non-zero multiple of 65536 (its own FIXME).  The summary below reports
 * the true answer: nonzero == 0 exactly when every quantised sample of the codeblock is zero.
 * schro_encoder_clean_up_transform is not part of this (it clears nothing for a real picture, :3417-3424). */
typedef struct {
  uint32_t nonzero;             /* quantised values != 0 in the codeblock: 0 = zero codeblock; the sum over a sub-band's
                                 * records is its zero flag (schro_encoder_quantise_subband's return, :3784) */
  uint32_t max_abs;             /* largest |q|: picks the 1 / 2 / 4-byte hand-over width (SchroHipCodeblock.src_bytes) */
} SchroHipCodeblockSummary;

/* the workgroup size of the DC recurrence: a band's anti-diagonal longer than this is walked in strides */
#define SCHRO_HIP_QUANTISE_DC_THREADS 256
/* ... and the most rows a DC band may have (two diagonals + the one being written live in LDS, indexed by row) */
#define SCHRO_HIP_QUANTISE_DC_MAX_ROWS 4096

typedef struct {
  void *coeffs;                 /* the component's coefficient plane (device, s16 or s32): read, reconstruction written back */
  void *quant;                  /* the quantised values (device), the SAME layout: a record's offsets and strides hold in both */
  size_t bytes;                 /* what each of the two planes spans: no record may reach past it; the planes may not overlap */
  const SchroHipCodeblock *codeblocks;  /* HOST array: dst_offset, dst_stride, width, height, quant_index; src_* ignored */
  int ncodeblocks;
  int is_intra;                 /* schro_table_offset_1_2, else _3_8 */
  int dc_predict_first;         /* > 0: the first dc_predict_first records are sub-band 0 of an intra picture and take the
                                 * DC recurrence; they share one dst_stride and tile ... */
  int dc_width, dc_height;      /* ... this rectangle at the plane's base, each sample in exactly one of them */
  SchroHipCodeblockSummary *summary;    /* device, ncodeblocks entries: cleared and filled by the call */
} SchroHipQuantPlane;

/* One launch of quantise_kernel for all planes of the call (unlike sizes and indices mix), one of quantise_dc_kernel
 * (a workgroup per plane) where planes ask for DC prediction.  Refused with SCHRO_HIP_EINVAL before anything is launched,
 * the message naming plane and record: a quant index above 60, bytes_per_sample not 2 or 4, a record of non-positive
 * width or height, a stride shorter than a row or not a multiple of the sample size, `quant` overlapping `coeffs`, a record
 * reaching outside `bytes`, DC records that do not tile the band.  (Only schro_hipframe_quantise, whose layouts of tiny
 * sub-bands contain records of no width or height, skips those: their summary is zero.) */
int schro_hip_quantise_batch (SchroHipContext * ctx, const SchroHipQuantPlane * planes, int nplanes, int bytes_per_sample);

/* ---- encoder: core-syntax transform data in the VLC parse codes, written on the device ---------
 *
 * schro_encoder_encode_transform_data (schroencoder.c:3462-3483) for params->is_noarith, that is
 * schro_encoder_encode_subband_noarith (:4072-4192) over component 0 .. 2 and sub-band 0 .. 3 * depth, WITHOUT its
 * quantiser call (:4100-4104): schro_hip_quantise_batch / schro_hipframe_quantise have run, the quant planes are the
 * input.  The output is what the reference appends to frame->pack from a synchronised pack, up to and including one
 * final schro_pack_sync.  Per sub-band: sync, uint (length); when length > 0, uint (quant index of codeblock (0, 0)),
 * sync and `length` bytes of the flushed sub-pack -- per codeblock in raster order bit (zero) when there is more than one
 * codeblock and index > 0, sint (0) when there is more than one codeblock and codeblock_mode_index == 1 (the ENCODER's
 * rule; schro_decoder_setup_codeblocks ignores the count), then schro_pack_encode_sint of every value, rows top to
 * bottom (schropack.c:148-178: 1 .. 32 bits on s16, up to 64 on s32).  Codeblock counts and rectangles are
 * schro_hip_codeblock_layout's: sub-band 0 takes entry [0], every other one [SCHRO_SUBBAND_SHIFT (position) + 1].
 *
 * Three things of the reference's are kept as they are.
 * (a) The zero test of s16 frames, schro_frame_data_is_zero (:4043-4070): true when the 16-bit wrapped sum of the 16-bit
 *     abs of every row is 0 (abs (-32768) stays -32768).  A codeblock's flag applies it to the codeblock's row pieces, the
 *     sub-band's flag to the sub-band's whole rows; each can be true over non-zero values, and the two can disagree in
 *     both directions.  The bytes follow the reference; false_zero_* count what was called zero though it holds a
 *     non-zero value -- codeblocks (of sub-bands that are written, where a flag is written) and sub-bands -- so that a
 *     caller sees that the stream and its local decode have parted.  s32 frames take the true test.
 *     SchroHipCodeblockSummary.nonzero keeps its true meaning; this call does not read the summaries.
 * (b) subband_bits is frame->actual_subband_bits: 8 x the difference of whole-byte offsets after the leading sync and
 *     before any trailing one -- 0 for a zero sub-band (its one bit is still in the accumulator), header + payload else.
 * (c) The quant offset written is always 0, so the records of one sub-band must carry one quant index.
 *
 * INT_MIN in an s32 plane is undefined in the reference (-value overflows); here it takes the 64-bit code of magnitude
 * 2^31 and stays inside the bound.  Bit positions are 32-bit: a picture whose schro_hip_noarith_encode_bound reaches 2^29
 * bytes is refused.  `capacity` may be any size; only min (capacity, bytes) bytes of `out` are ever written. */
#define SCHRO_HIP_NOARITH_MAX_SUBBANDS 19       /* 1 + 3 * SCHRO_HIP_LIMIT_TRANSFORM_DEPTH */
typedef struct {
  uint32_t bytes;               /* what the picture takes, whether or not it fitted */
  uint32_t overrun;             /* 1: bytes > capacity, `out` holds the first `capacity` bytes */
  uint32_t false_zero_codeblocks, false_zero_subbands;  /* (a) */
  uint32_t subband_bits[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];     /* (b); entries past 3 * depth are 0 */
} SchroHipNoarithResult;

typedef struct {
  const void *quant[3];         /* device: Y, U, V quant planes (s16 or s32); not written */
  size_t bytes[3];              /* what each plane spans: no record may reach past it */
  int stride[3];                /* bytes between rows of the plane */
  int iwt_width[3], iwt_height[3];      /* the transform's size: positive multiples of 1 << transform_depth */
  const SchroHipCodeblock *codeblocks[3];       /* HOST: schro_hip_codeblock_layout's records for `stride`; quant_index read */
  int ncodeblocks[3];
  int transform_depth;
  int horiz_codeblocks[7], vert_codeblocks[7];  /* params->horiz_codeblocks / vert_codeblocks [0 .. depth] */
  int codeblock_mode_index;
  uint8_t *out;                 /* device: the bytes */
  size_t capacity;              /* of out */
  SchroHipNoarithResult *result;        /* device, 4-byte aligned: cleared and filled by the call */
} SchroHipNoarithPicture;

/* The capacity that always suffices: 4 bytes per s16 sample or 8 per s32 sample, two flag bits per codeblock and ten
 * bytes of header and padding per sub-band.  Reads the sizes, the depth and the counts of `picture` only; < 0 on refusal. */
int64_t schro_hip_noarith_encode_bound (const SchroHipNoarithPicture * picture, int bytes_per_sample);

/* Pictures of unlike geometry in one call: a count launch over all row pieces (a codeblock's part of a sub-band row), a
 * layout launch (a workgroup per picture), a clear of the bytes the picture takes and a pack launch.  Enqueues, does not
 * synchronise.  Refused (SCHRO_HIP_EINVAL, nothing enqueued, the message naming picture, component and sub-band or
 * record): bytes_per_sample not 2 or 4, a depth above 6, sizes that are no positive multiples of 1 << depth or reach
 * 32768, codeblock counts outside 1 .. 32767, a codeblock_mode_index other than 0 / 1, a NULL or misaligned pointer, a
 * stride shorter than a row or no multiple of the sample size, records that are not schro_hip_codeblock_layout's for the
 * stated counts and stride, a record that reaches outside `bytes`, a quant index above 60, unlike quant indices in one
 * sub-band, a bound of 2^29 bytes or more, an output that overlaps a quant plane. */
int schro_hip_noarith_encode_batch (SchroHipContext * ctx, const SchroHipNoarithPicture * pictures, int npictures,
    int bytes_per_sample);
/* host only: the refusals of schro_hip_noarith_encode_batch without a context.  No pointer is dereferenced but the HOST arrays. */
int schro_hip_noarith_encode_check (const SchroHipNoarithPicture * pictures, int npictures, int bytes_per_sample);

/* ---- decoder: core-syntax transform data in the VLC parse codes, read on the device ------------
 *
 * schro_decoder_parse_transform_data (schrodecoder.c:2939-2987) and schro_decoder_decode_transform_data (:2990-3015,
 * :3279-3449, :3525-3625) for params->is_noarith: the picture's transform-data bytes go in, from a synchronised position;
 * the completely filled, dequantised coefficient planes come out.  A sub-band of length 0 is zero-filled, a codeblock whose
 * zero flag is set is zero-filled, every other sample is dequantised with the decoder's arithmetic (s16 planes: the 16-bit
 * Orc program; s32 planes: C int -- the same two forms schro_hip_dequant_batch has).  Arithmetic-coded pictures take
 * schro_hip_arith_decode_batch, further down.
 *
 * These are the DECODER's rules; the encoder's (schro_hip_noarith_encode_batch above) differ.  Per component and sub-band
 * the outer unpack reads: byte sync, uint (length); length 0: byte sync; else uint (quant index), byte sync and `length`
 * bytes of payload, which its own unpack reads with guard bit 1 (bits past the payload's end read as 1, so every further
 * value is 0).  have_zero_flags = more than one codeblock, for EVERY sub-band (the encoder writes none for sub-band 0);
 * have_quant_offset = codeblock_mode_index == 1 && !(compat_quant_offset && one codeblock) (the encoder writes an offset
 * only where there is more than one codeblock).  Per codeblock, in raster order over schro_hip_codeblock_layout's
 * rectangles: bit (zero) when have_zero_flags; quant index += sint, clamped to 0 .. 60 (clamped_quant counts) and carried
 * to the next codeblock, when have_quant_offset; width x height sints, rows top to bottom.  The two rule sets agree where
 * sub-band 0 has one codeblock and either the mode is 0 or compat_quant_offset is set.
 *
 * schro_decoder_test_quant_offset_compat (:3324-3352): in sub-band 0 of each component, when it is coded, has one
 * codeblock and have_quant_offset holds, quant index + (a peeked sint) outside 0 .. 60 sets the decoder INSTANCE's
 * compat_quant_offset: from then on no sub-band of one codeblock has an offset, that one included, in later components and
 * later pictures.  The call takes the state before the picture and reports the state after it.
 *
 * Where the reference is undefined the call is defined and bounded.  The input is fetched as the aligned dwords that hold
 * its bytes (so up to 3 bytes in front of `data` and behind its end are loaded, masked and never used); nothing else is read:
 *  - schro_unpack_decode_uint computes 1 << count, undefined from count 31 on.  Here v = 1; per data bit v = (v << 1 | b)
 *    mod 2^32; the magnitude is v - 1 mod 2^32; a code with data bits always has a sign bit; then the sign, then truncation
 *    to the sample type.  Equal to the reference for every code an encoder can write (count <= 30); the others are
 *    counted in long_codes (headers, offsets and values; not the compat test's peek).
 *  - a header quant index above 60 (picture->error, :2971): error = 1, first_error = component * 19 + index, NOTHING of the
 *    picture's planes is written, compat_quant_offset is reported as it came in, the header fields stand as far as the
 *    walk went.  Other pictures of the call are unaffected.
 *  - a length that reaches past the input's end: the payload is cut there and decoded with guard bits; `truncated` counts
 *    such sub-bands (the reference would read outside its buffer).
 *  - what the reference only warns about (:3606-3622): sub-bands with bits_read / 8 < length - 1 count in not_consumed,
 *    with bits_read / 8 > length in overran (length as stated). */
typedef struct {
  uint32_t bytes_read;          /* whole bytes the outer unpack consumed (rounded up; saturates at 2^32 - 1) */
  uint32_t error, first_error;  /* quant index > 60 in a header: nothing written */
  uint32_t compat_quant_offset; /* the instance's state after this picture */
  uint32_t truncated, not_consumed, overran, long_codes, clamped_quant;
  uint32_t subband_length[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];
  uint8_t subband_quant_index[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];       /* of codeblock (0,0), as the header states it */
} SchroHipNoarithDecodeResult;

typedef struct {
  const uint8_t *data;          /* device: the transform data, from a synchronised position */
  size_t data_bytes;            /* host: at most this many bytes are ever used (below 2^29) */
  const uint32_t *bytes_on_device;      /* optional, device, 4-byte aligned: min (*bytes_on_device, data_bytes) is the length --
                                           e.g. &SchroHipNoarithResult.bytes of an encode on the same queue */
  void *coeffs[3];              /* device: Y, U, V coefficient planes (s16 or s32) */
  size_t bytes[3];              /* what each plane spans */
  int stride[3];                /* bytes between rows, of coeffs and of quant */
  void *quant[3];               /* optional, same layout: the values as read, not dequantised (all three or none) */
  int iwt_width[3], iwt_height[3], transform_depth;
  int horiz_codeblocks[7], vert_codeblocks[7], codeblock_mode_index;
  int is_intra;                 /* num_refs == 0: offsets _1_2, else _3_8.  The LL bands are NOT DC-predicted here: an error
                                   picture must stay untouched and the error is only known on the device, so the caller runs
                                   schro_hip_dc_predict_batch once result->error is known (schro_hipframe_decode_transform_data_noarith does) */
  int compat_quant_offset;      /* the instance's state before this picture */
  SchroHipNoarithDecodeResult *result;  /* device, 4-byte aligned: cleared and filled by the call */
} SchroHipNoarithDecodePicture;

/* Pictures of unlike geometry and depth in one call: a header launch (the serial chain of at most 57 sub-band headers
 * per picture), a summary launch (a lane per 64-bit chunk of every payload), a chain launch (a workgroup per coded
 * sub-band finds every codeblock's first bit by composing the summaries), a decode launch (a lane per chunk decodes,
 * dequantises and stores the codes that start in it) and a fill launch (zero sub-bands, zero codeblocks, values behind
 * the payload's end).  Enqueues, does not synchronise; bytes between a row's width and the stride and everything outside
 * the planes are not written.  Refused (SCHRO_HIP_EINVAL, nothing enqueued, the message naming picture and component):
 * bytes_per_sample not 2 or 4, a depth above 6, sizes that are no positive multiples of 1 << depth or reach 32768,
 * codeblock counts outside 1 .. 32767, a codeblock_mode_index other than 0 / 1, a NULL or misaligned pointer, a stride
 * shorter than a row or no multiple of the sample size, a plane that does not hold its rows, `data` overlapping a plane,
 * `quant` overlapping `coeffs`, `result` overlapping `data`, `bytes_on_device` or a plane, planes overlapping each other,
 * anything one picture of the call writes (planes, result) overlapping what another reads or writes (the results are
 * cleared in front of the first launch), data_bytes of 2^29 or more. */
int schro_hip_noarith_decode_batch (SchroHipContext * ctx, const SchroHipNoarithDecodePicture * pictures, int npictures,
    int bytes_per_sample);
/* host only: the refusals of schro_hip_noarith_decode_batch without a context.  No pointer is dereferenced. */
int schro_hip_noarith_decode_check (const SchroHipNoarithDecodePicture * pictures, int npictures, int bytes_per_sample);
/* host only: the words of queue scratch the call takes for these pictures (5 per chunk slot -- data_bytes / 8 + sub-bands
 * + 1 slots per picture --, 3 per codeblock, 8 per sub-band, 2 per picture), or < 0 on refusal. */
int64_t schro_hip_noarith_decode_scratch_words (const SchroHipNoarithDecodePicture * pictures, int npictures, int bytes_per_sample);

/* ---- decoder: arithmetic-coded core-syntax transform data, read on the device -------------------
 *
 * schro_decoder_parse_transform_data (schrodecoder.c:2939-2987) and schro_decoder_decode_transform_data (:2990-3015) for
 * !params->is_noarith -- the form every default encoder writes: schro_decoder_decode_subband (:3525-3638) over
 * schro_decoder_decode_codeblock (:3452-3522), the generic line decoder (:3018-3217; its three _p_ forms compute the same)
 * and the binary arithmetic decoder (schroarith.h:147-210, schroarith.c:211-239, 283-288, 642-668).  The headers, the
 * codeblock counts and rectangles, have_zero_flags, have_quant_offset and the state compat_quant_offset are those of the
 * VLC call above; only the payloads differ.
 *
 * The coder: range 0xffff0000, the code is the payload's first four bytes (0xff for a byte that does not exist), offset
 * 3, cntr 16, every probability 0x8000 per sub-band.  A bin renormalises while range <= 0x40000000 -- two bytes enter every
 * 16 shifts, 0xff behind the payload's end --, then range_x_prob = ((range >> 16) * p) & 0xffff0000, bit = code >=
 * range_x_prob, and p moves by the 256-entry table.  uint: bits = 1; while the continuation bin is 0: bits = bits << 1 |
 * (data bin), the continuation context moves on; the value is (int) (bits - 1).  The quant offset is a sint whose loop also
 * stops after 30 data bins.  Per coefficient the continuation context comes from parent != 0 (sub-band index - 3 at
 * (x >> 1, y >> 1), from position 4 on) and from the OR of the left, upper and upper-left values; the sign context from
 * the left value (horizontally oriented bands), the upper value (vertically oriented) or none -- each the STORED value,
 * dequantised and truncated to the sample type.  A non-zero value v is stored as +- ((offset + factor * v + 2) >> 2) in C
 * int for both sample sizes (NOT the 16-bit Orc form of the VLC path), offsets _1_2 when is_intra, else _3_8.
 *
 * schro_decoder_test_quant_offset_compat peeks a sint with a COPY of the fresh coder of sub-band 0 (one codeblock, an
 * offset, coded); otherwise as above.  The LL band of an intra picture is NOT DC-predicted here (as above).
 *
 * Where the reference is undefined the call is defined and bounded; the input is fetched as the aligned dwords that hold
 * its bytes and nothing else is read:
 *  - a uint of 32 or more data bins wraps: bits is kept mod 2^32 (a wrapped value of 0 has no sign bin, as the reference's
 *    `if (v)`); from 31 data bins on (int) (bits - 1) is negative.  Codes of 31 or more data bins count in long_codes.
 *  - offset + factor * v + 2 past 2^31: 32-bit two's-complement wrap, an arithmetic shift, a wrapping negation.  This is
 *    what the x86-64 build of the reference computes; it is undefined in C and NOT pinned against the reference.
 *  - quant index + offset is formed in 64 bits and clamped to 0 .. 60 (clamped_quant counts).
 *  - a header quant index above 60, a length past the input's end (the payload goes on with 0xff bytes, the reference's
 *    own rule for the end of a buffer): as above.
 *  - after a sub-band schro_arith_decode_flush; offset < length - 1 counts in not_consumed, offset > length + 4 in overran.
 * Running time is bounded by the input alone: see DESIGN 4.24. */
typedef struct {
  uint32_t bytes_read;          /* whole bytes the outer unpack consumed (rounded up; saturates at 2^32 - 1) */
  uint32_t error, first_error;  /* quant index > 60 in a header: nothing written */
  uint32_t compat_quant_offset; /* the instance's state after this picture */
  uint32_t truncated, not_consumed, overran, long_codes, clamped_quant;
  uint32_t subband_length[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];
  uint8_t subband_quant_index[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];       /* of codeblock (0,0), as the header states it */
  uint32_t bins;                /* binary decisions decoded for the picture (the compat peeks not counted; saturates at 2^32 - 1) */
} SchroHipArithDecodeResult;

/* The fields of SchroHipNoarithDecodePicture with the same meanings. */
typedef struct {
  const uint8_t *data;          /* device: the transform data, from a synchronised position */
  size_t data_bytes;            /* host: at most this many bytes are ever used (below 2^29) */
  const uint32_t *bytes_on_device;      /* optional, device, 4-byte aligned: min (*bytes_on_device, data_bytes) is the length */
  void *coeffs[3];              /* device: Y, U, V coefficient planes (s16 or s32) */
  size_t bytes[3];              /* what each plane spans */
  int stride[3];                /* bytes between rows, of coeffs and of quant */
  void *quant[3];               /* optional, same layout: the values as read, not dequantised (all three or none) */
  int iwt_width[3], iwt_height[3], transform_depth;
  int horiz_codeblocks[7], vert_codeblocks[7], codeblock_mode_index;
  int is_intra;                 /* num_refs == 0: offsets _1_2, else _3_8; no DC prediction (see above) */
  int compat_quant_offset;      /* the instance's state before this picture */
  SchroHipArithDecodeResult *result;    /* device, 4-byte aligned: cleared and filled by the call */
} SchroHipArithDecodePicture;

/* Pictures of unlike geometry and depth in one call: a header launch (the serial chain of sub-band headers per picture,
 * with the compat peeks), a clear launch (the planes of every picture without the error, so that zero sub-bands and zero
 * codeblocks read as zero to their children and neighbours) and a decode launch.  Its unit is the TOWER: sub-band i >= 4
 * reads sub-band i - 3, so a component is four serial chains -- LL, and per orientation the levels from coarse to fine --
 * and a picture twelve; a wave decodes a tower, one lane deciding, one bin per trip of its loop.  Enqueues, does not synchronise; bytes
 * between a row's width and the stride and everything outside the planes are not written.  The refusals are those of
 * schro_hip_noarith_decode_batch. */
int schro_hip_arith_decode_batch (SchroHipContext * ctx, const SchroHipArithDecodePicture * pictures, int npictures,
    int bytes_per_sample);
/* host only: the refusals of schro_hip_arith_decode_batch without a context.  No pointer is dereferenced. */
int schro_hip_arith_decode_check (const SchroHipArithDecodePicture * pictures, int npictures, int bytes_per_sample);
/* host only: the words of queue scratch the call takes for these pictures (8 per sub-band), or < 0 on refusal. */
int64_t schro_hip_arith_decode_scratch_words (const SchroHipArithDecodePicture * pictures, int npictures, int bytes_per_sample);

/* ---- encoder: the motion data of a noarith (VLC) picture, written on the device ----------------
 *
 * What schro_encoder_encode_picture appends to frame->pack between the prediction parameters and the transform
 * parameters (schroencoder.c:2505-2515) for params->is_noarith, from a synchronised pack: the sections superblock split,
 * prediction modes, ref-1 x, ref-1 y, with two references ref-2 x and ref-2 y, and the DC of Y, U, V
 * (schro_encoder_encode_superblock_split, _prediction_modes, _vector_data, _dc_data, :2841-3142) -- 7 or 9 of them, each
 * sync, uint (payload bytes), sync, the flushed sub-pack; an empty section is the one byte 0x80.  Section indices are
 * always 0 split, 1 modes, 2 / 3 ref-1 x / y, 4 / 5 ref-2 x / y, 6 .. 8 DC; with one reference 4 and 5 are absent.
 *
 * `motion` is a field of SchroMotionVector records (20 bytes: pred_mode : 2, using_global : 1, split : 2 in the first
 * word; dx[2], dy[2] -- or dc[3] -- at byte 12), x_num_blocks * y_num_blocks of them in raster order: what
 * schro_hip_mode_decision_batch leaves in its `motion`.  Superblocks go in raster order, the units of one in steps of
 * 4 >> split of its top-left record.  The predictions (schromotion.c:163-430) read the neighbours' records as they are:
 * nothing checks that a split-0 or split-1 superblock carries the copies schro_motion_verify (:441-525) demands, and a
 * field without them codes to bytes that decode to another field.  `unverified` counts the blocks schro_motion_verify
 * would reject -- a split unlike the superblock's, a copy of a split-0 / split-1 superblock that is not byte-equal to its
 * origin, a DC outside -128 .. 127, pred_mode >= 2 with one reference, using_global without have_global_motion --
 * and first_unverified is the raster index of the first one (-1: none).  `asserted` counts where the reference asserts:
 * a superblock of split 3 (coded as split 2 here: the reference would not terminate) and a coded unit with using_global
 * though have_global_motion is 0.  When it is not 0 the bytes are unspecified; the call still ends inside its buffers. */
#define SCHRO_HIP_MOTION_SECTIONS 9
typedef struct {
  uint32_t bytes;               /* what the picture takes, whether or not it fitted */
  uint32_t overrun;             /* 1: bytes > capacity, `out` holds the first `capacity` bytes */
  uint32_t section_bytes[SCHRO_HIP_MOTION_SECTIONS];    /* the payload of each section; absent and empty ones 0 */
  uint32_t section_units[SCHRO_HIP_MOTION_SECTIONS];    /* the units each section codes (modes: every coded unit) */
  uint32_t asserted;
  uint32_t unverified;
  int32_t first_unverified;
} SchroHipMotionEncodeResult;

typedef struct {
  const void *motion;           /* device, 4-byte aligned: the records; not written */
  int x_num_blocks, y_num_blocks;       /* positive multiples of 4, at most 16384 */
  int num_refs;                 /* 1 or 2 */
  int have_global_motion;
  uint8_t *out;                 /* device: the bytes */
  size_t capacity;              /* of out */
  SchroHipMotionEncodeResult *result;   /* device, 4-byte aligned: every word written by the call */
} SchroHipMotionEncodePicture;

/* The capacity that always suffices.  A vector or DC difference of two int16 takes at most 34 bits (magnitude <= 65535:
 * 33 bits of uint code and a sign); a block carries four of them with two references, or three DCs -- and with one
 * reference two vector components or three DCs: 136 or 102 bits; its mode takes 1 + (num_refs > 1) + (have_global_motion
 * != 0) bits; a superblock's split residual (0 .. 2) at most 3 bits.  A section adds less than a byte of padding behind
 * its payload and at most 8 bytes of length code (59 bits below 2^29) with its padding: 9 bytes for each of the 7 or 9.
 *   bound = (blocks * (136 | 102 + mode bits) + superblocks * 3 + 7) / 8 + 9 * sections
 * < 0 on refusal (block counts, num_refs). */
int64_t schro_hip_motion_encode_bound (int x_num_blocks, int y_num_blocks, int num_refs, int have_global_motion);

/* Pictures of unlike geometry and num_refs in one call: a count launch (a lane per block, the 16 lanes of a row one
 * superblock), a layout launch (a workgroup per picture), a clear of the bytes the picture takes and a pack launch.
 * Enqueues, does not synchronise; the tables come from the queue's grow-only scratch.  Behind
 * schro_hip_mode_decision_batch on the same queue it takes that call's `motion` as it is.  Refused (SCHRO_HIP_EINVAL,
 * nothing enqueued, the message naming the picture): block counts that are no positive multiples of 4 or above 16384,
 * num_refs other than 1 / 2, a NULL or misaligned pointer, an output or result that overlaps the field or another
 * picture's buffers, a bound of 2^29 bytes or more.  Only min (capacity, bytes) bytes of `out` are ever written. */
int schro_hip_motion_encode_batch (SchroHipContext * ctx, const SchroHipMotionEncodePicture * pictures, int npictures);
/* host only: the refusals of schro_hip_motion_encode_batch without a context.  No pointer is dereferenced. */
int schro_hip_motion_encode_check (const SchroHipMotionEncodePicture * pictures, int npictures);

/* ---- decoder: the motion data of a noarith (VLC) picture, read on the device -------------------
 *
 * The twin of schro_decoder_parse_block_data and schro_decoder_decode_block_data / _decode_macroblock /
 * _decode_prediction_unit (schrodecoder.c:2531-2814) for params->is_noarith: the bytes above, from a synchronised
 * position, to the field of 20-byte records schro_hip_obmc_batch reads.  The output is what the reference leaves after
 * orc_splat_u8_ns (.., 0, ..) and the decode: the flags, the slots the block's mode names -- three DCs, or the vector of
 * each reference the mode names unless the block is global -- and everything else 0: a global block's four vector
 * slots, the metrics, the padding.
 *
 * Hostile input is defined; there is no error picture: every byte string decodes to a field.
 *   - Bits behind a section's kept payload read 1 (schro_unpack_init_with_data (.., 1)).
 *   - Header, per section: byte_sync, uint, byte_sync.  The length is taken mod 2^32 and cut at the input's end
 *     (`truncated`); a header that starts behind the input reads guard bits and gives length 0.
 *   - schro_unpack_decode_uint is undefined from 31 data bits on.  Here, as for the transform data: v = 1;
 *     v = (v << 1 | b) mod 2^32 per data bit, the value is v - 1 mod 2^32; a signed code with data bits always has a
 *     sign bit.  Codes of 31 or more data bits are counted in long_codes: those of the headers, and in every section
 *     but the modes those among the codes the section can be asked for at all -- its first x * y codes, x * y / 16 for
 *     the splits --, whether the field asked for them or not.
 *   - Vectors and DCs are (int16_t) (pred + value): the wrap is invisible.  A split is (pred + value) % 3 with value
 *     in 0 .. 2^32 - 1 and an addition that does not wrap again: split 3 cannot arise.
 *   - Input bytes are fetched as the aligned 32-bit words that hold at least one byte of data[0 .. data_bytes); no
 *     value depends on the other bytes of such a word.  Nothing outside `motion` and `result` is written. */
typedef struct {
  uint32_t bytes;               /* the position behind the last section, cut at the input */
  uint32_t section_bytes[SCHRO_HIP_MOTION_SECTIONS];    /* the payload as kept (4 and 5 are 0 with one reference) */
  uint32_t section_units[SCHRO_HIP_MOTION_SECTIONS];    /* the codes the field asked of the section (1: coded units) */
  uint32_t section_bits[SCHRO_HIP_MOTION_SECTIONS];     /* the bits read from it, guard bits included (at most 2^32 - 1) */
  uint32_t truncated;           /* masks, bit s for section s: the stated length reached past the input */
  uint32_t overran;             /* section_bits > 8 * section_bytes */
  uint32_t not_consumed;        /* a whole byte or more was left unread */
  uint32_t long_codes;          /* a count, see above */
  uint32_t unverified;          /* blocks schro_motion_verify rejects: in a decoded field, a DC outside -128 .. 127 */
  int32_t first_unverified;     /* the raster index of the first one, or -1 */
} SchroHipMotionDecodeResult;

typedef struct {
  const uint8_t *data;          /* device, any alignment: the bytes from a synchronised position */
  size_t data_bytes;            /* below 2^29 */
  const uint32_t *bytes_on_device;      /* or NULL: a device word; min (word, data_bytes) bytes are read
                                           (e.g. SchroHipMotionEncodeResult.bytes on the same queue) */
  int x_num_blocks, y_num_blocks;       /* positive multiples of 4, at most 16384 */
  int num_refs;                 /* 1 or 2 */
  int have_global_motion;
  void *motion;                 /* device, 4-byte aligned: x * y records of 20 bytes, every byte written */
  SchroHipMotionDecodeResult *result;   /* device, 4-byte aligned, every word written */
} SchroHipMotionDecodePicture;

/* Pictures of unlike geometry, num_refs and global flag in one call.  Seven launches: header (a lane per picture walks
 * the 7 or 9 section headers), summary (a lane per 64-bit chunk of sections 0 and 2 .. 8), scan (a workgroup per section
 * composes the summaries: entry state and first code index per chunk), extract (a lane per chunk stores the codes that
 * start in it as 32-bit residuals by index), and three walks of one workgroup per picture over anti-diagonals -- splits
 * over superblocks, then modes and then vectors / DCs over blocks --, each followed by the prefix sums the next one
 * needs.  With have_global_motion the mode section is a serial chain (a unit's third bit exists only when its mode is not
 * 0): one lane walks it in stream order.  Enqueues, does not synchronise; the tables come from the queue's grow-only
 * scratch.  Refused (SCHRO_HIP_EINVAL, nothing enqueued, the message naming the picture): block counts that are no
 * positive multiples of 4 or above 16384, num_refs other than 1 / 2, NULL data, motion or result, a misaligned motion,
 * result or bytes_on_device, data_bytes of 2^29 or more, motion or result overlapping data, bytes_on_device or each
 * other, anything one picture writes overlapping what another picture of the call reads or writes. */
int schro_hip_motion_decode_batch (SchroHipContext * ctx, const SchroHipMotionDecodePicture * pictures, int npictures);
/* host only: the refusals of schro_hip_motion_decode_batch without a context.  No pointer is dereferenced. */
int schro_hip_motion_decode_check (const SchroHipMotionDecodePicture * pictures, int npictures);
/* host only: the words of queue scratch the call takes, or < 0 on refusal.  Per picture of b blocks and c = (data_bytes
 * + 7) / 8 + 8 chunk slots: 72 (the sections) + 4 c (summary, entry) + 3 b / 16 rounded up to even (split residuals,
 * splits, first units) + 10 b (seven residual arrays, flags, two code indices). */
int64_t schro_hip_motion_decode_scratch_words (const SchroHipMotionDecodePicture * pictures, int npictures);

/* ---- decoder: the motion data of an arithmetic-coded picture, read on the device ----------------
 *
 * The same twin (schrodecoder.c:2531-2814) for !params->is_noarith: the same headers in front of nine arithmetic-coded
 * payloads, one coder per section (schro_arith_decode_init, every probability 0x8000).  The field is byte for byte what
 * schro_hip_motion_decode_batch leaves for the same values: the flags, the slots the block's mode names, everything
 * else 0.
 *
 * No bin's context depends on a decoded neighbour: a split is _schro_arith_decode_uint (SB_F1 -> SB_F2 -> SB_F2 ..,
 * SB_DATA), a mode bit one bin in BLOCK_MODE_REF1 / _REF2 (and GLOBAL_BLOCK), a vector residual _schro_arith_decode_sint
 * over CONT_BIN1 .. CONT_BIN5 (the last repeats), VALUE, SIGN, a DC residual over CONT_BIN1, CONT_BIN2, VALUE, SIGN; the
 * sint loop stops after 30 data bins.  So a section's k-th value is the same whatever the field is, and only how many
 * values a section is asked for depends on the field: each section is one serial chain of bins, and the three walks of
 * schro_hip_motion_decode_batch run between the chains.
 *
 * Hostile input is defined; there is no error picture: every byte string decodes to a field.
 *   - The header walk is schro_hip_motion_decode_batch's, rule for rule: byte_sync, uint, byte_sync; the length mod 2^32,
 *     cut at the input's end (`truncated`); a header behind the input reads guard bits and gives length 0.
 *   - The bin is schro_hip_arith_decode_batch's: range 0xffff0000, code = the first four payload bytes, 0xff where the
 *     kept payload is shorter; renormalise while range <= 0x40000000, two bytes every 16 shifts, 0xff behind the payload;
 *     ((range >> 16) * p) & 0xffff0000 decides.
 *   - A uint keeps `bits` mod 2^32 and its value is bits - 1 mod 2^32.  Codes of 31 or more data bins are counted in
 *     long_codes: those of the header lengths and the splits (the sint loop stops at 30).
 *   - A split is (pred + value) % 3 with value in 0 .. 2^32 - 1 and an addition that does not wrap again.  Vectors and
 *     DCs are (int16_t) (pred + value).
 *   - Input bytes are fetched as the aligned 32-bit words that hold at least one byte of data[0 .. data_bytes); no
 *     value depends on the other bytes of such a word.  Nothing outside `motion` and `result` is written.
 * Running time is bounded by the input alone: a coder decides at most about 1500 bins per payload byte,
 * about 3000 behind the payload's end, and then one bin per value asked. */
typedef struct {
  uint32_t bytes;               /* the position behind the last section, cut at the input */
  uint32_t section_bytes[SCHRO_HIP_MOTION_SECTIONS];    /* the payload as kept (4 and 5 are 0 with one reference) */
  uint32_t section_units[SCHRO_HIP_MOTION_SECTIONS];    /* the values the field asked of the section (1: coded units) */
  uint32_t section_offset[SCHRO_HIP_MOTION_SECTIONS];   /* the coder's `offset` behind the last bin asked: 3 if none was, 0 for an absent section */
  uint32_t section_bins[SCHRO_HIP_MOTION_SECTIONS];     /* the bins decided (at most 2^32 - 1) */
  uint32_t truncated;           /* masks, bit s for section s: the stated length reached past the input */
  uint32_t overran;             /* offset > stated length + 6 (schrodecoder.c:2598) */
  uint32_t not_consumed;        /* offset < stated length (:2594); no flush is involved */
  uint32_t long_codes;          /* a count, see above */
  uint32_t unverified;          /* blocks schro_motion_verify rejects: in a decoded field, a DC outside -128 .. 127 */
  int32_t first_unverified;     /* the raster index of the first one, or -1 */
} SchroHipMotionArithDecodeResult;

typedef struct {
  const uint8_t *data;          /* device, any alignment: the bytes from a synchronised position */
  size_t data_bytes;            /* below 2^29 */
  const uint32_t *bytes_on_device;      /* or NULL: a device word; min (word, data_bytes) bytes are read */
  int x_num_blocks, y_num_blocks;       /* positive multiples of 4, at most 16384 */
  int num_refs;                 /* 1 or 2 */
  int have_global_motion;
  void *motion;                 /* device, 4-byte aligned: x * y records of 20 bytes, every byte written */
  SchroHipMotionArithDecodeResult *result;      /* device, 4-byte aligned, every word written */
} SchroHipMotionArithDecodePicture;

/* Pictures of unlike geometry, num_refs and global flag in one call.  Seven launches: header (a lane per picture walks
 * the 7 or 9 section headers), the split chain (a wave per picture, one lane deciding: x * y / 16 uints), the split walk,
 * the mode chain (a wave per picture: units * (1 + (num_refs > 1)) bins), the mode walk, the value chains (a wave per
 * section 2 .. 8 and picture: section_units sints) and the value walk -- the walks as in schro_hip_motion_decode_batch.
 * With have_global_motion the third mode bin exists only when the unit's mode is not 0: the mode chain does nothing and
 * one lane of the mode walk predicts and decodes the units in stream order (correct and slow).  Enqueues, does not
 * synchronise; the tables come from the queue's grow-only scratch.  Refused as schro_hip_motion_decode_batch refuses, in
 * the same words. */
int schro_hip_motion_arith_decode_batch (SchroHipContext * ctx, const SchroHipMotionArithDecodePicture * pictures, int npictures);
/* host only: the refusals of schro_hip_motion_arith_decode_batch without a context.  No pointer is dereferenced. */
int schro_hip_motion_arith_decode_check (const SchroHipMotionArithDecodePicture * pictures, int npictures);
/* host only: the words of queue scratch the call takes, or < 0 on refusal.  Per picture of b blocks: 36 (the sections)
 * + 3 b / 16 rounded up to even (split residuals, splits, first units) + 11 b (the mode bins by unit, seven residual
 * arrays, flags, two code indices). */
int64_t schro_hip_motion_arith_decode_scratch_words (const SchroHipMotionArithDecodePicture * pictures, int npictures);

/* ---- encoder: sub-band histograms on the device ----------------------------------------------
 *
 * The pass over the coefficients that every rate-controlled quantiser choice starts with
 * (schro_encoder_generate_subband_histograms, schroquantiser.c:600-637): per sub-band, how many of its SAMPLED values --
 * rows 0, skip, 2 skip ... < height, all columns -- fall into each of the 104 logarithmic bins of ilogx
 * (schrohistogram.c:11-22): x = |v|, halved while x >= 16, i halvings, bin x + 8 i -- so |v| itself below 16, then 8
 * bins per octave, bins 0 .. 103 covering |v| <= 32767.
 *   plain form (schro_frame_data_generate_histogram, :345-357): the value counted is the coefficient;
 *   DC-predict form (schro_frame_data_generate_histogram_dc_predict with x = y = 0, :359-391): the value counted is
 *     line[i] - pred, pred from the ORIGINAL neighbours (no recurrence): 0 at (0, 0), line[i - 1] on row 0,
 *     prev_line[i] in column 0, otherwise schro_divide3 (line[i - 1] + prev_line[i] + prev_line[i - 1] + 1) =
 *     (a * 21845 + 10922) >> 16; prev_line is row j - 1 of the band, not the previous sampled row.  The form starts at
 *     the band's own row 0: nothing above the band is read.
 *   s32 planes (the reference reads s16 only): the same expressions in 32-bit wrapping ints, so that values within 16
 *     bits give the s16 result.
 * The counts are RAW: the reference's scale by skip (schro_histogram_scale) is the caller's, or
 * schro_hipframe_subband_histograms'.
 * One departure, deliberate: the reference indexes bins[ilogx (v)] without a bound -- a coefficient of -32768 lands on
 * index 104, the DC form's differences reach +-65535, index 111, and both write past its array.  Here every sample whose
 * index is >= 104 is counted in `overflow` and the 104 bins are left alone; the reference's n counts those samples, and so
 * does bins[...] + overflow here. */
#define SCHRO_HIP_HISTOGRAM_BINS 104
typedef struct {
  uint32_t bins[SCHRO_HIP_HISTOGRAM_BINS];
  uint32_t overflow;
} SchroHipHistogramCounts;      /* raw counts, before the scale by skip */
typedef struct {
  int offset, stride, width, height;    /* bytes from `coeffs` to sample (0, 0), bytes between rows, samples, samples */
  int skip;                     /* a power of two >= 1: rows 0, skip, 2 skip ... are counted */
  int dc_predict;               /* the DC-predict form */
} SchroHipHistogramBand;
typedef struct {
  const void *coeffs;           /* the component's coefficient plane (device, s16 or s32): read, never written */
  size_t bytes;                 /* what it spans: no band may reach past it */
  const SchroHipHistogramBand *bands;   /* HOST array */
  int nbands;
  SchroHipHistogramCounts *counts;      /* device, nbands entries: cleared and filled by the call */
} SchroHipHistogramPlane;

/* One launch of histogram_kernel for every band of every plane of the call (unlike sizes, skips and forms mix).  Refused
 * with SCHRO_HIP_EINVAL before anything is launched, the message naming plane and band: bytes_per_sample not 2 or 4, a
 * non-positive width or height, a skip that is not a power of two >= 1, a stride shorter than a row or not a multiple of
 * the sample size, a band reaching outside `bytes` (an offset in front of the plane included: the DC form's row 0 has no
 * row above it to read, and none is read), a band of 2^32 or more sampled values.  Enqueued on the selected queue; the
 * counts are complete once that queue has passed the call. */
int schro_hip_histogram_batch (SchroHipContext * ctx, const SchroHipHistogramPlane * planes, int nplanes, int bytes_per_sample);

/* ---- encoder: the quantiser choice on the device ------------------------------------------------
 *
 * What every rate-controlled engine of the reference does with the histograms above, without a host step:
 * schro_encoder_calc_estimates (schroquantiser.c:688-732) and then schro_encoder_lambda_to_entropy (:838-885) once
 * (rdo_lambda, rdo_cbr: :758-782), under schro_encoder_entropy_to_lambda's search and once more at its answer
 * (rdo_bit_allocation, :738-756, :887-969), or schro_encoder_lambda_to_error under schro_encoder_error_to_lambda's
 * search (constant_error, :971-1119).  The input is the three components' SchroHipHistogramCounts arrays as
 * schro_hip_histogram_batch leaves them, on the same queue; the output is a device record whose quant_index rows
 * schro_hip_quantise_chosen_batch reads.
 *
 * Estimates: per (component, sub-band, index j < 60) est_entropy = schro_histogram_estimate_entropy (hist, j, is_noarith)
 * * context_ratio and est_error = schro_histogram_apply_table (hist, error table j) (schrohistogram.c:42-104, :266-343,
 * schroutils.c:309-327), on bins = counts * skip as doubles, in the reference's evaluation order, nothing fused.  What no
 * transcendental touches is the reference's bit for bit: est_error, the twelve ranges, the sub-band lambdas, frame_lambda.
 * The device's exp and log are within 1 ulp, as the host's are: est_entropy agrees with a host's to parts in 10^16 (the
 * noarith branch: |d (1 - exp (-12.5 r))| < 4e-16 is a relative 3e-17 / r of the estimate, r = bin[1] / bin[0] >= 2^-32)
 * and is not promised as bits.  The premise of the exact part: a sub-band's counts sum to less than 2^32 (as
 * schro_hip_histogram_batch guarantees) and skip <= 1024, so that every sum inside get_range is exact in a double.
 *
 * The reference's behaviour, kept: all 104 bins zero (every sampled value in `overflow`, or an empty band) makes the
 * noarith estimate 0 / 0 = NaN for every index, and index 0 is chosen (NaN never satisfies x < min); the first minimum
 * wins; the sub-band lambda is frame lambda, *= subband0 scale, *= chroma scale, *= diagonal scale, /= weight * weight
 * in that order, the error path without the diagonal scale; constant_error leaves the indices of its LAST evaluation and
 * never evaluates at the lambda it returns, bit allocation evaluates once more at its answer; lo == hi after the steps
 * returns sqrt (lo * hi) at once.  not_bracketed is the condition of the reference's "not bracketed" message; its own
 * control flow never makes it true (a search that runs out of steps ends in lo == hi, or in NaN sums that compare false).
 *
 * The tables are encoder state and the caller's: encoder->intra_hist_tables (60 x 104 weights) and, for pictures that
 * are not noarith, the one-bits / zero-bits tables of the same shape.  The sub-band weights
 * (encoder->intra_ / inter_subband_weights [filter][MAX (0, depth - 1)]), the arith context ratios and the three
 * magic_*_lambda_scale travel with each picture. */
#define SCHRO_HIP_QUANT_CHOOSE_INDICES 60
#define SCHRO_HIP_QUANT_ENGINE_LAMBDA 0           /* target: the frame lambda (rdo_lambda, rdo_cbr) */
#define SCHRO_HIP_QUANT_ENGINE_BIT_ALLOCATION 1   /* target: frame->allocated_residual_bits */
#define SCHRO_HIP_QUANT_ENGINE_CONSTANT_ERROR 2   /* target: the error, 255 * 0.1 ^ (0.05 noise_threshold) * width * height */
typedef struct {
  double frame_lambda;          /* the lambda engine's target, or what the search returned */
  double sum;                   /* what the last evaluation returned: entropy, or (constant error) error */
  double chosen_entropy[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];     /* the estimates at quant_index; a host forms */
  double chosen_error[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];       /* estimated_residual_bits from them (:785-798) */
  int32_t quant_index[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];       /* what the engine leaves; entries past 3 * depth are 0 */
  int32_t evaluations;          /* lambda_to_entropy / _error calls made */
  int32_t not_bracketed;
  int32_t reserved;
} SchroHipQuantChoice;

typedef struct {
  const SchroHipHistogramCounts *counts[3];     /* device: 1 + 3 * transform_depth entries per component; not written */
  int skip[SCHRO_HIP_NOARITH_MAX_SUBBANDS];     /* per sub-band, what the histogram call sampled with: 1 .. 1024, a power of two */
  int transform_depth;          /* 0 .. 6 */
  int is_intra;                 /* 0 / 1; the tables the reference picks by it are the caller's: weights and ratios below */
  int is_noarith;               /* which branch of the entropy estimate */
  int engine;                   /* SCHRO_HIP_QUANT_ENGINE_* */
  double subband_weight[SCHRO_HIP_NOARITH_MAX_SUBBANDS];        /* finite, positive */
  double context_ratio[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];
  double subband0_lambda_scale, chroma_lambda_scale, diagonal_lambda_scale;
  double target;
  SchroHipQuantChoice *result;  /* device, 8-byte aligned: every byte written */
  double *est_entropy, *est_error;      /* device or NULL: [3][19][60] doubles each, the rows of sub-bands past 3 * depth untouched */
} SchroHipQuantChoosePicture;

/* The tables into device memory of the context (stored [104][60]: the 60 lanes of an estimate read neighbours).
 * error: 60 x 104 doubles; onebits, zerobits: the same shape, or both NULL.  Calling it again replaces them; it waits for
 * the context's queues first. */
int schro_hip_quant_choose_tables (SchroHipContext * ctx, const double *error, const double *onebits, const double *zerobits);
/* Pictures of unlike depth, form and engine in one call, two launches: the estimates (a wave per component and sub-band,
 * lane j owns index j) and the choice (a workgroup per picture runs the whole engine, search included).  Enqueues, does
 * not synchronise; the estimates go through the queue's grow-only scratch.  Refused (SCHRO_HIP_EINVAL, nothing enqueued,
 * the message naming the picture and the field): what schro_hip_quant_choose_check refuses, no tables, more than 65535
 * pictures. */
int schro_hip_quant_choose_batch (SchroHipContext * ctx, const SchroHipQuantChoosePicture * pictures, int npictures);
/* host only: a depth outside 0 .. 6, a skip that is no power of two in 1 .. 1024, a weight that is not finite and
 * positive, a non-finite ratio, scale or target, an unknown engine, is_intra / is_noarith other than 0 / 1, NULL or
 * misaligned pointers, a picture that is not noarith when have_bit_tables is 0.  No pointer is dereferenced. */
int schro_hip_quant_choose_check (const SchroHipQuantChoosePicture * pictures, int npictures, int have_bit_tables);

/* The two consumers with the indices taken from device memory, so that histograms -> choice -> quantise -> bytes is one
 * run of enqueued calls.  Everything is schro_hip_quantise_batch's / schro_hip_noarith_encode_batch's -- structs,
 * refusals, kernels, results bit for bit -- but for this: a codeblock record's quant_index holds its SUB-BAND number
 * (0 .. 3 * depth), and the index comes from chosen[plane][sub-band] (the quantiser: a device row of 19 int32 per plane,
 * SchroHipQuantChoice.quant_index[component]) or chosen[picture][component][sub-band] (the VLC encoder: a device block
 * of 3 x 19 int32 per picture, SchroHipQuantChoice.quant_index).  `chosen` itself is a HOST array of device pointers.  A
 * small resolve launch behind the job table's upload writes the constants the host would have written.  A value outside
 * 0 .. 60 -- it can only come from a table of the caller's own making -- is clamped into range and counted: *clamped, a
 * device word the caller has cleared, is added to once per record (quantiser) or sub-band (VLC encoder) that read one.
 * One index per sub-band: the VLC encoder's refusal of unlike indices in a sub-band cannot arise.  Refused in addition:
 * a NULL or misaligned chosen[.] or clamped, a record whose quant_index is not a sub-band (above 18; the VLC encoder: not
 * the sub-band its place in the layout says). */
int schro_hip_quantise_chosen_batch (SchroHipContext * ctx, const SchroHipQuantPlane * planes, const int32_t * const *chosen, int nplanes,
    int bytes_per_sample, uint32_t * clamped);
int schro_hip_noarith_encode_chosen_batch (SchroHipContext * ctx, const SchroHipNoarithPicture * pictures, const int32_t * const *chosen,
    int npictures, int bytes_per_sample, uint32_t * clamped);
/* host only: the refusals of schro_hip_noarith_encode_chosen_batch without a context.  No pointer is dereferenced but the HOST arrays. */
int schro_hip_noarith_encode_chosen_check (const SchroHipNoarithPicture * pictures, const int32_t * const *chosen, int npictures,
    int bytes_per_sample, const uint32_t * clamped);

/* ---- frame layer: the reference's stage boundary ------------------------- */

/* The structs of this layer are LAYOUT-IDENTICAL to the reference's (same members, same
 * order, same offsets on LP64): a SchroFrame * / SchroParams * / SchroMotion * /
 * SchroMemoryDomain * of schroedinger 1.0.11 can be passed where this header says
 * SchroHipFrame * / SchroHipParams * / SchroHipMotion * / SchroHipMemoryDomain *.  The offsets
 * below were recorded from the reference's own headers by scripts/ref_layout.py
 * (tests/golden/ref_layout.json) and are pinned here by _Static_assert; where the
 * reference's headers are present, tests/c/layout_check.c compares member by member. */

#define SCHRO_HIP_FRAME_CACHE_SIZE 32   /* SCHRO_FRAME_CACHE_SIZE, schroframe.h:56 */
#define SCHRO_HIP_LIMIT_TRANSFORM_DEPTH 6       /* schrolimits.h:50 */
#define SCHRO_HIP_LIMIT_BLOCK_SIZE 64   /* schrolimits.h:67 */
#define SCHRO_HIP_MEMORY_DOMAIN_SLOTS 1000      /* schrodomain.h:11 */
/* schrodomain.h:34-36 defines CPU 0x1, CUDA 0x2, OPENGL 0x4; the next free bit */
#define SCHRO_MEMORY_DOMAIN_HIP 0x0008

/* SchroMemoryDomain (schrodomain.h:13-28): the reference's slot cache
 * (schro_memory_domain_alloc, schrodomain.c:58-137) calls alloc / free of this table, so
 * schro_frame_new_and_alloc (domain, ...) (schroframe.c:172-188) hands out device frames
 * when `domain` came from schro_memory_domain_new_hip.  alloc / free take no domain argument
 * (the reference's signature): they use the HIP domain of the calling thread's current
 * device.  The members after `slots` are private to this library. */
typedef struct _SchroHipMemoryDomain {
  void *mutex;                  /* SchroMutex *: the reference host creates and owns it */
  unsigned int flags;           /* SCHRO_MEMORY_DOMAIN_HIP */
  void *(*alloc) (int size);
  void *(*alloc_2d) (int depth, int width, int height);
  void (*free) (void *ptr, int size);
  struct {
    unsigned int flags;
    void *ptr;
    int size;
    void *priv;
  } slots[SCHRO_HIP_MEMORY_DOMAIN_SLOTS];
  /* -- end of the reference's struct -- */
  SchroHipContext *ctx;
} SchroHipMemoryDomain;

/* schro_memory_domain_new_cuda (schrocuda.h:9) replacement: a context on `device` (its queues,
 * caches) behind a SchroMemoryDomain-shaped handle.  schro_hip_domain_context gives the context
 * for the plane-layer calls; schro_memory_domain_free_hip releases both. */
SchroHipMemoryDomain *schro_memory_domain_new_hip (int device);
void schro_memory_domain_free_hip (SchroHipMemoryDomain * domain);
/* a domain of PINNED HOST memory (flags SCHRO_MEMORY_DOMAIN_CPU): see schro_hip_host_alloc; free it with free () */
SchroHipMemoryDomain *schro_memory_domain_new_hip_host (void);
SchroHipContext *schro_hip_domain_context (SchroHipMemoryDomain * domain);
/* the domain of a context made with schro_hip_context_new */
SchroHipMemoryDomain *schro_hip_context_domain (SchroHipContext * ctx);

/* SchroFrameData (schroframe.h:58-67) */
typedef struct {
  int format;                   /* SchroFrameFormat */
  void *data;
  int stride;
  int width;
  int height;
  int length;
  int h_shift;
  int v_shift;
} SchroHipFrameData;

/* SchroFrame (schroframe.h:69-94).  domain == NULL: host memory; a HIP domain: `data` of
 * every component is a device pointer.  An upsampled device frame (is_upsampled) holds the
 * tiled half-pel images in its components and keeps its integer-pel source frame in
 * virt_frame1. */
typedef struct _SchroHipFrame SchroHipFrame;
struct _SchroHipFrame {
  int refcount;
  void (*free) (SchroHipFrame * frame, void *priv);
  SchroHipMemoryDomain *domain;
  void *regions[3];
  void *priv;

  int format;
  int width;
  int height;

  SchroHipFrameData components[3];

  int is_virtual;
  int cached_lines[3][SCHRO_HIP_FRAME_CACHE_SIZE];
  SchroHipFrame *virt_frame1;
  SchroHipFrame *virt_frame2;
  void (*render_line) (SchroHipFrame * frame, void *dest, int component, int i);
  void *virt_priv;
  void *virt_priv2;

  int extension;
  int cache_offset[3];
  int is_upsampled;
  int upsample_done;            /* schro_bool */
};

/* SchroGlobalMotion, SchroParams (schroparams.h:18-74) */
typedef struct {
  int b0, b1, a_exp, a00, a01, a10, a11, c_exp, c0, c1;
} SchroHipGlobalMotion;

typedef struct {
  void *video_format;           /* SchroVideoFormat * */
  int is_noarith;
  int wavelet_filter_index;
  int transform_depth;
  int horiz_codeblocks[SCHRO_HIP_LIMIT_TRANSFORM_DEPTH + 1];
  int vert_codeblocks[SCHRO_HIP_LIMIT_TRANSFORM_DEPTH + 1];
  int codeblock_mode_index;
  int num_refs;
  int have_global_motion;
  int xblen_luma;
  int yblen_luma;
  int xbsep_luma;
  int ybsep_luma;
  int mv_precision;
  SchroHipGlobalMotion global_motion[2];
  int picture_pred_mode;
  int picture_weight_bits;
  int picture_weight_1;
  int picture_weight_2;
  int is_lowdelay;
  int n_horiz_slices;
  int n_vert_slices;
  int slice_bytes_num;
  int slice_bytes_denom;
  int quant_matrix[3 * SCHRO_HIP_LIMIT_TRANSFORM_DEPTH + 1];
  int iwt_chroma_width;
  int iwt_chroma_height;
  int iwt_luma_width;
  int iwt_luma_height;
  int x_num_blocks;
  int y_num_blocks;
  int x_offset;
  int y_offset;
} SchroHipParams;

/* SchroMotion (schromotion.h:53-86); schro_motion_render_hip reads src1, src2,
 * motion_vectors and params, as schro_motion_render_u8 does (schromotion8.c:700-730) */
typedef struct {
  SchroHipFrame *src1;          /* device; plain u8 if mv_precision == 0 else upsampled */
  SchroHipFrame *src2;          /* may be NULL */
  void *motion_vectors;         /* HOST SchroMotionVector array (schromotion.h:20-37) */
  SchroHipParams *params;
  int ref_weight_precision;
  int ref1_weight;
  int ref2_weight;
  int mv_precision;
  int xoffset;
  int yoffset;
  int xbsep;
  int ybsep;
  int xblen;
  int yblen;
  SchroHipFrameData block;
  SchroHipFrameData alloc_block;
  SchroHipFrameData obmc_weight;
  SchroHipFrameData alloc_block_ref[2];
  SchroHipFrameData block_ref[2];
  int weight_x[SCHRO_HIP_LIMIT_BLOCK_SIZE];
  int weight_y[SCHRO_HIP_LIMIT_BLOCK_SIZE];
  int width;
  int height;
  int max_fast_x;
  int max_fast_y;
  int simple_weight;            /* schro_bool */
  int oneref_noscale;
} SchroHipMotion;

#if defined(__LP64__) || defined(_LP64)
#include <stddef.h>
#ifdef __cplusplus
#define SCHRO_HIP_LAYOUT(t, m, off) static_assert (offsetof (t, m) == (off), #t "." #m)
#define SCHRO_HIP_SIZE(t, n) static_assert (sizeof (t) == (n), #t)
#else
#define SCHRO_HIP_LAYOUT(t, m, off) _Static_assert (offsetof (t, m) == (off), #t "." #m)
#define SCHRO_HIP_SIZE(t, n) _Static_assert (sizeof (t) == (n), #t)
#endif
/* numbers: tests/golden/ref_layout.json (scripts/ref_layout.py, from the reference's headers) */
SCHRO_HIP_SIZE (SchroHipFrameData, 40);
SCHRO_HIP_LAYOUT (SchroHipFrameData, data, 8);
SCHRO_HIP_LAYOUT (SchroHipFrameData, stride, 16);
SCHRO_HIP_LAYOUT (SchroHipFrameData, v_shift, 36);
SCHRO_HIP_SIZE (SchroHipFrame, 648);
SCHRO_HIP_LAYOUT (SchroHipFrame, free, 8);
SCHRO_HIP_LAYOUT (SchroHipFrame, domain, 16);
SCHRO_HIP_LAYOUT (SchroHipFrame, regions, 24);
SCHRO_HIP_LAYOUT (SchroHipFrame, priv, 48);
SCHRO_HIP_LAYOUT (SchroHipFrame, format, 56);
SCHRO_HIP_LAYOUT (SchroHipFrame, width, 60);
SCHRO_HIP_LAYOUT (SchroHipFrame, height, 64);
SCHRO_HIP_LAYOUT (SchroHipFrame, components, 72);
SCHRO_HIP_LAYOUT (SchroHipFrame, is_virtual, 192);
SCHRO_HIP_LAYOUT (SchroHipFrame, cached_lines, 196);
SCHRO_HIP_LAYOUT (SchroHipFrame, virt_frame1, 584);
SCHRO_HIP_LAYOUT (SchroHipFrame, render_line, 600);
SCHRO_HIP_LAYOUT (SchroHipFrame, extension, 624);
SCHRO_HIP_LAYOUT (SchroHipFrame, is_upsampled, 640);
SCHRO_HIP_LAYOUT (SchroHipFrame, upsample_done, 644);
SCHRO_HIP_SIZE (SchroHipParams, 336);
SCHRO_HIP_LAYOUT (SchroHipParams, wavelet_filter_index, 12);
SCHRO_HIP_LAYOUT (SchroHipParams, transform_depth, 16);
SCHRO_HIP_LAYOUT (SchroHipParams, num_refs, 80);
SCHRO_HIP_LAYOUT (SchroHipParams, have_global_motion, 84);
SCHRO_HIP_LAYOUT (SchroHipParams, xblen_luma, 88);
SCHRO_HIP_LAYOUT (SchroHipParams, mv_precision, 104);
SCHRO_HIP_LAYOUT (SchroHipParams, picture_weight_bits, 192);
SCHRO_HIP_LAYOUT (SchroHipParams, is_lowdelay, 204);
SCHRO_HIP_LAYOUT (SchroHipParams, slice_bytes_num, 216);
SCHRO_HIP_LAYOUT (SchroHipParams, quant_matrix, 224);
SCHRO_HIP_LAYOUT (SchroHipParams, iwt_chroma_width, 300);
SCHRO_HIP_LAYOUT (SchroHipParams, iwt_luma_width, 308);
SCHRO_HIP_LAYOUT (SchroHipParams, x_num_blocks, 316);
SCHRO_HIP_LAYOUT (SchroHipParams, y_offset, 328);
SCHRO_HIP_LAYOUT (SchroHipMemoryDomain, flags, 8);
SCHRO_HIP_LAYOUT (SchroHipMemoryDomain, alloc, 16);
SCHRO_HIP_LAYOUT (SchroHipMemoryDomain, alloc_2d, 24);
SCHRO_HIP_LAYOUT (SchroHipMemoryDomain, free, 32);
SCHRO_HIP_LAYOUT (SchroHipMemoryDomain, slots, 40);
SCHRO_HIP_LAYOUT (SchroHipMemoryDomain, ctx, 32040);
SCHRO_HIP_LAYOUT (SchroHipMotion, motion_vectors, 16);
SCHRO_HIP_LAYOUT (SchroHipMotion, params, 24);
SCHRO_HIP_LAYOUT (SchroHipMotion, ref_weight_precision, 32);
SCHRO_HIP_SIZE (SchroHipSubpelChain, 88);
SCHRO_HIP_LAYOUT (SchroHipSubpelChain, ref_up, 16);
SCHRO_HIP_LAYOUT (SchroHipSubpelChain, width, 28);
SCHRO_HIP_LAYOUT (SchroHipSubpelChain, mv_precision, 56);
SCHRO_HIP_LAYOUT (SchroHipSubpelChain, lambda, 64);
SCHRO_HIP_LAYOUT (SchroHipSubpelChain, field, 80);
SCHRO_HIP_SIZE (SchroHipSplit2Picture, 184);
SCHRO_HIP_LAYOUT (SchroHipSplit2Picture, num_refs, 36);
SCHRO_HIP_LAYOUT (SchroHipSplit2Picture, ref_up, 40);
SCHRO_HIP_LAYOUT (SchroHipSplit2Picture, width, 100);
SCHRO_HIP_LAYOUT (SchroHipSplit2Picture, mv_precision, 136);
SCHRO_HIP_LAYOUT (SchroHipSplit2Picture, lambda, 144);
SCHRO_HIP_LAYOUT (SchroHipSplit2Picture, motion, 168);
SCHRO_HIP_SIZE (SchroHipModeTrial, 24);
SCHRO_HIP_LAYOUT (SchroHipModeTrial, score, 16);
SCHRO_HIP_SIZE (SchroHipModePicture, 232);
SCHRO_HIP_LAYOUT (SchroHipModePicture, hbm_fields, 184);
SCHRO_HIP_LAYOUT (SchroHipModePicture, trials, 216);
SCHRO_HIP_LAYOUT (SchroHipModePicture, stats, 224);
SCHRO_HIP_SIZE (SchroHipMotionEncodeResult, 92);
SCHRO_HIP_LAYOUT (SchroHipMotionEncodeResult, section_units, 44);
SCHRO_HIP_LAYOUT (SchroHipMotionEncodeResult, first_unverified, 88);
SCHRO_HIP_SIZE (SchroHipMotionEncodePicture, 48);
SCHRO_HIP_LAYOUT (SchroHipMotionEncodePicture, num_refs, 16);
SCHRO_HIP_LAYOUT (SchroHipMotionEncodePicture, out, 24);
SCHRO_HIP_LAYOUT (SchroHipMotionEncodePicture, result, 40);
SCHRO_HIP_SIZE (SchroHipMotionDecodeResult, 136);
SCHRO_HIP_LAYOUT (SchroHipMotionDecodeResult, section_bits, 76);
SCHRO_HIP_LAYOUT (SchroHipMotionDecodeResult, truncated, 112);
SCHRO_HIP_LAYOUT (SchroHipMotionDecodeResult, first_unverified, 132);
SCHRO_HIP_SIZE (SchroHipMotionDecodePicture, 56);
SCHRO_HIP_LAYOUT (SchroHipMotionDecodePicture, bytes_on_device, 16);
SCHRO_HIP_LAYOUT (SchroHipMotionDecodePicture, num_refs, 32);
SCHRO_HIP_LAYOUT (SchroHipMotionDecodePicture, motion, 40);
SCHRO_HIP_LAYOUT (SchroHipMotionDecodePicture, result, 48);
SCHRO_HIP_SIZE (SchroHipMotionArithDecodeResult, 172);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodeResult, section_offset, 76);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodeResult, section_bins, 112);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodeResult, truncated, 148);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodeResult, first_unverified, 168);
SCHRO_HIP_SIZE (SchroHipMotionArithDecodePicture, 56);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodePicture, bytes_on_device, 16);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodePicture, num_refs, 32);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodePicture, motion, 40);
SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodePicture, result, 48);
SCHRO_HIP_SIZE (SchroHipArithDecodeResult, 328);
SCHRO_HIP_LAYOUT (SchroHipArithDecodeResult, clamped_quant, 32);
SCHRO_HIP_LAYOUT (SchroHipArithDecodeResult, subband_length, 36);
SCHRO_HIP_LAYOUT (SchroHipArithDecodeResult, subband_quant_index, 264);
SCHRO_HIP_LAYOUT (SchroHipArithDecodeResult, bins, 324);
SCHRO_HIP_SIZE (SchroHipArithDecodePicture, 216);
SCHRO_HIP_LAYOUT (SchroHipArithDecodePicture, bytes_on_device, 16);
SCHRO_HIP_LAYOUT (SchroHipArithDecodePicture, stride, 72);
SCHRO_HIP_LAYOUT (SchroHipArithDecodePicture, quant, 88);
SCHRO_HIP_LAYOUT (SchroHipArithDecodePicture, transform_depth, 136);
SCHRO_HIP_LAYOUT (SchroHipArithDecodePicture, codeblock_mode_index, 196);
SCHRO_HIP_LAYOUT (SchroHipArithDecodePicture, result, 208);
SCHRO_HIP_SIZE (SchroHipUnpackPicture, 120);
SCHRO_HIP_LAYOUT (SchroHipUnpackPicture, src_stride, 24);
SCHRO_HIP_LAYOUT (SchroHipUnpackPicture, format, 36);
SCHRO_HIP_LAYOUT (SchroHipUnpackPicture, src_bpp, 48);
SCHRO_HIP_LAYOUT (SchroHipUnpackPicture, dst, 64);
SCHRO_HIP_LAYOUT (SchroHipUnpackPicture, dst_bpp, 100);
SCHRO_HIP_LAYOUT (SchroHipUnpackPicture, width, 112);
SCHRO_HIP_SIZE (SchroHipUnpackIwtPicture, 88);
SCHRO_HIP_LAYOUT (SchroHipUnpackIwtPicture, format, 12);
SCHRO_HIP_LAYOUT (SchroHipUnpackIwtPicture, width, 24);
SCHRO_HIP_LAYOUT (SchroHipUnpackIwtPicture, dst, 32);
SCHRO_HIP_LAYOUT (SchroHipUnpackIwtPicture, iwt_width, 68);
SCHRO_HIP_LAYOUT (SchroHipUnpackIwtPicture, h_shift, 76);
#endif

/* schro_frame_new_and_alloc (schroframe.c:60-191) on the device domain:
 * planar Y,U,V, stride = round-up-64 (width * bytes); upsampled == 1
 * allocates 2w x 2h half-pel images per component. */
SchroHipFrame *schro_hip_frame_new_and_alloc (SchroHipContext * ctx,
    int format, int width, int height, int upsampled);
SchroHipFrame *schro_hip_frame_ref (SchroHipFrame * frame);
void schro_hip_frame_unref (SchroHipFrame * frame);

/* schro_frame_to_gpu / schro_gpuframe_to_cpu (schrogpuframe.h:17-18):
 * whole-frame copies, all three components, synchronous on return. */
int schro_frame_to_hip (SchroHipFrame * dest, SchroHipFrame * src);
int schro_hipframe_to_cpu (SchroHipFrame * dest, SchroHipFrame * src);
/* r03: the same, enqueued on the context's selected queue and NOT waited for (see the asynchronous
 * transfers above: host frames in pinned memory, queues 2 / 3, marks, schro_hip_queue_synchronize) */
int schro_frame_to_hip_async (SchroHipFrame * dest, SchroHipFrame * src);
int schro_hipframe_to_cpu_async (SchroHipFrame * dest, SchroHipFrame * src);
/* a copy of a device frame (plain or upsampled) on another context's device: one hipMemcpyPeerAsync per
 * component on dst_ctx's selected queue, complete on return (the scheduler's reference migration) */
SchroHipFrame *schro_hip_frame_copy_to (SchroHipContext * dst_ctx, SchroHipFrame * src);

/* How the stage calls below end.  complete_on_return != 0 (the default): the reference's contract -- a stage
 * is complete when its function returns (schroasync-pthread.c:320-328); the call waits for the selected
 * queue.  0: the calls only ENQUEUE on the selected queue (frames must be on the device already; the
 * motion vectors go through pinned staging buffers), for a host that keeps several pictures in flight and
 * orders them with marks (0.58 ms per 2160p picture, host hand-over included, against 0.98 ms
 * under the contract). */
int schro_hip_context_set_stage_completion (SchroHipContext * ctx, int complete_on_return);

/* schro_gpuframe_iwt_transform (schrogpuframe.h:13-31) replacement: the forward wavelet of all three components of
 * `frame` (device, s16 or s32) IN PLACE, with params->wavelet_filter_index and transform_depth over iwt_luma_* /
 * iwt_chroma_*: the source planes are copied into the queue's scratch first, then schro_hip_iwt_batch's launches. */
int schro_hipframe_iwt_transform (SchroHipContext * ctx, SchroHipFrame * frame, const SchroHipParams * params);

/* One pyramid level of schro_encoder_frame_downsample (schroanalysis.c:24-25): schro_frame_downsample (dest, src) plus,
 * when dest->extension > 0, schro_frame_mc_edgeextend (dest), all three components in one launch.  Both frames are u8
 * device frames of one domain; every component of dest is (w + 1) / 2 x (h + 1) / 2 of src's, its data pointer at pixel
 * (0, 0) with dest->extension samples of apron around it (schro_frame_new_and_alloc_extended's layout). */
int schro_hipframe_downsample (SchroHipFrame * dest, SchroHipFrame * src);
/* schro_rough_me_heirarchical_scan_nohint (schroroughmotion.c:64-141; the spelling is the reference's) over the luma
 * planes of two u8 device frames that are both ALREADY at pyramid level `shift`.  motion_vectors: a HOST array of
 * params->x_num_blocks x params->y_num_blocks SchroMotionVector records; every record is set as schro_motion_field_set
 * (mf, 0, 1) leaves it, the blocks at multiples of 1 << shift receive dx << shift, dy << shift in dx[ref], dy[ref] and
 * the metric (a scan of no width or height: 0, 0, INT_MAX).  Synchronises: the array is complete on return. */
int schro_rough_me_heirarchical_scan_nohint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame,
    const SchroHipParams * params, int shift, int distance, int ref, void *motion_vectors);

/* schro_rough_me_heirarchical_scan_hint (schroroughmotion.c:143-300) over the luma planes of two u8 device frames that
 * are both at pyramid level `shift`.  hint_motion_vectors: the HOST field of level shift + 1 (read); motion_vectors: the
 * HOST field of level `shift` (every record written).  The fields cross to the device and back through the queue's
 * scratch.  Synchronises: the array is complete on return. */
int schro_rough_me_heirarchical_scan_hint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame,
    const SchroHipParams * params, int shift, int distance, int ref, const void *hint_motion_vectors, void *motion_vectors);
/* schro_rough_me_heirarchical_scan (schroroughmotion.c:47-62): frames[k], ref_frames[k] are the u8 device frames at
 * pyramid level k as get_downsampled (:303-312) returns them, motion_fields[k] the HOST field of level k, for k = 1 ..
 * n_levels (entry 0 of the three arrays is not read).  The nohint level at distance 12, the hint levels at distance 4
 * (:58-60), one launch; the fields stay on the device between the levels and are downloaded together.  Synchronises
 * once, at the end. */
int schro_rough_me_heirarchical_scan_hip (SchroHipFrame * const *frames, SchroHipFrame * const *ref_frames,
    const SchroHipParams * params, int n_levels, int ref, void *const *motion_fields);

/* schro_hierarchical_bm_scan_hint (schrohierbm.c:174-383) over all three components of two u8 device frames of one
 * chroma format that are both at pyramid level `shift` (0: the full pictures).  hint_motion_vectors: the HOST field of
 * level shift + 1 (read), or NULL at the top level; motion_vectors: the HOST field of level `shift` (every record
 * written).  frame->extension must be at least max (xbsep_luma, ybsep_luma).  The fields cross to the device and back
 * through the queue's scratch.  Synchronises: the array is complete on return. */
int schro_hierarchical_bm_scan_hint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame,
    const SchroHipParams * params, int shift, int h_range, int ref, const void *hint_motion_vectors, void *motion_vectors);
/* schro_hbm_scan (schrohierbm.c:158-172) and, with_level0, the level-0 call of schro_encoder_motion_predict_pel
 * (schromotionest.c:123-127): frames[k], ref_frames[k] are the u8 device frames at pyramid level k, motion_fields[k] the
 * HOST field of level k, for k = 0 .. n_levels (without with_level0 entry 0 of the three arrays is not read).  One
 * launch; the fields stay on the device between the levels and are downloaded together.  Synchronises once, at the
 * end. */
int schro_hbm_scan_hip (SchroHipFrame * const *frames, SchroHipFrame * const *ref_frames,
    const SchroHipParams * params, int n_levels, int ref, int with_level0, void *const *motion_fields);

/* schro_encoder_motion_predict_subpel_deep (schromotionest.c:246-354): src -- the u8 device frame of the picture,
 * ref_upframes -- params->num_refs (1 or 2) upsampled device frames (schro_upsampled_hipframe_upsample), subpel_fields --
 * as many HOST fields of params->x_num_blocks * params->y_num_blocks records, each holding the level-0 field of its
 * reference (schro_encoder_predict_subpel_picture's copy, schroencoder.c:2307-2317) and refined in place to
 * params->mv_precision; field r refines dx[r], dy[r].  src->extension must lie in max (xbsep_luma, ybsep_luma) .. 32.  The
 * fields cross to the device and back through the queue's scratch, the references are the chains of one
 * schro_hip_subpel_batch.  One wait, at the end. */
int schro_encoder_motion_predict_subpel_deep_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes,
    const SchroHipParams * params, double lambda, void *const *subpel_fields);
/* The split-2 level of schro_mode_decision (schromotionest.c:2587-2688; schro_hip_split2_batch above): src -- the u8
 * device frame of the picture, ref_upframes -- params->num_refs (1 or 2) upsampled device frames of its format,
 * subpel_fields -- per reference the HOST sub-pel field (read), motion -- HOST memory for x_num_blocks * y_num_blocks
 * records, superblocks -- HOST memory for 16 bytes per superblock.  The chroma shifts are the frame format's, the
 * extension is src->extension.  One wait, at the end. */
int schro_mode_decision_split2_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes, const SchroHipParams * params, double lambda,
    const void *const *subpel_fields, void *motion, void *superblocks);
/* schro_mode_decision entire (schro_hip_mode_decision_batch above), the same arguments and: hbm_fields -- per reference
 * the HOST level-1 and level-2 fields of the block matching, hbm_fields[2 r] and hbm_fields[2 r + 1]; trials -- HOST
 * memory for four SchroHipModeTrial per superblock, or NULL; stats -- three doubles: mc_error, badblock_ratio,
 * dcblock_ratio.  One wait, at the end. */
int schro_mode_decision_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes, const SchroHipParams * params, double lambda,
    const void *const *subpel_fields, const void *const *hbm_fields, void *motion, void *superblocks, void *trials, double *stats);

/* schro_frame_inverse_iwt_transform_cuda (schrocuda.h:13-14) replacement, same arguments:
 * upload transform_frame (host) or use it where it is (device), run the multi-level inverse
 * transform into `frame` (device, iwt-padded size). */
int schro_frame_inverse_iwt_transform_hip (SchroHipFrame * frame,
    SchroHipFrame * transform_frame, SchroHipParams * params);
/* r04 -- the inverse transform and x_combine's add in one call: output_frame (device u8) = sat_u8 (inverse
 * transform of transform_frame + prediction), prediction = the frame schro_motion_render_hip (motion, dest, NULL,
 * FALSE, NULL) rendered (the mc_tmp_frame of the reference's GPU paths, schrodecoder.c:1742-1760, :1908-1921), or
 * NULL for a picture without references (+ 128, :1788-1790).  The residual picture never exists in memory. */
int schro_frame_inverse_iwt_transform_combine_hip (SchroHipFrame * output_frame, SchroHipFrame * transform_frame,
    SchroHipParams * params, SchroHipFrame * prediction);
/* r05: the same for a picture WITHOUT references whose output picture is v210 (BASELINE config 5): x_wavelet_transform and
 * the schro_frame_convert of x_combine (schrodecoder.c:2011-2052) in one call -- `packed` a device frame of format v210,
 * transform_frame a device s16 / s32 4:2:2 frame; schro_hipframe_to_cpu (output_picture, packed) follows.  Same bytes as
 * schro_frame_inverse_iwt_transform_hip + schro_hipframe_convert; the pixel frame is not written where
 * schro_hip_iiwt_pack_v210_batch's fused kernel applies. */
int schro_frame_inverse_iwt_transform_convert_hip (SchroHipFrame * packed, SchroHipFrame * transform_frame, SchroHipParams * params);
/* `packed` may also be a YUYV, UYVY or AYUV device frame (s16 or s32 transform frame of any chroma format the pack takes):
 * schro_hip_iiwt_pack_u8_batch.  And the same with a prediction: x_wavelet_transform, the add and x_combine's convert of
 * an inter picture that is not a reference (schrodecoder.c:1908-1921, :1969-2021) in one stage call -- prediction = the u8
 * frame schro_motion_render_hip (motion, dest, NULL, FALSE, NULL) rendered, as for
 * schro_frame_inverse_iwt_transform_combine_hip, with its domain and size checks; prediction == NULL is the call above.
 * Same bytes as schro_frame_inverse_iwt_transform_combine_hip + schro_hipframe_convert; a v210 `packed` takes no
 * prediction. */
int schro_frame_inverse_iwt_transform_combine_convert_hip (SchroHipFrame * packed, SchroHipFrame * transform_frame,
    SchroHipParams * params, SchroHipFrame * prediction);
/* `packed` may also be a v216, ARGB or AY64 device frame -- the formats of the > 8-bit pictures -- from an s16 / s32 transform
 * frame of the format's own chroma format (4:2:2 for v216, 4:4:4 for ARGB / AY64): schro_hip_iiwt_pack_wide_batch, same bytes as
 * schro_frame_inverse_iwt_transform_hip + schro_hipframe_convert.  With a prediction these formats are refused, like v210
 * (the reference has no > 8-bit inter path).
 * schro_frame_inverse_iwt_transform_shift_convert_hip is the whole non-reference intra tail of x_combine in one stage call:
 * x_wavelet_transform, schro_frame_shift_right (frame, shift) where the stream's bit depth exceeds the output picture's
 * (schrodecoder.c:2013-2019) and the convert -- same bytes as schro_frame_inverse_iwt_transform_hip +
 * schro_hipframe_shift_right + schro_hipframe_convert.  v216 / ARGB / AY64 take any shift in [0, 8 * bytes per sample); for
 * the other packed formats shift 0 is schro_frame_inverse_iwt_transform_convert_hip and another shift SCHRO_HIP_EINVAL. */
int schro_frame_inverse_iwt_transform_shift_convert_hip (SchroHipFrame * packed, SchroHipFrame * transform_frame,
    SchroHipParams * params, int shift);

/* schro_decoder_decode_lowdelay_transform_data (picture), schrolowdelay.c:746-762, with
 * picture->transform_frame on the device: `slices` is picture->lowdelay_buffer->data (host),
 * copied to the device compressed; the frame's format picks s16 / s32.  Synchronous. */
int schro_hip_decode_lowdelay_transform_data (SchroHipFrame * transform_frame,
    const void *slices, size_t slices_bytes, const SchroHipLowDelayParams * params);
/* schro_encoder_encode_lowdelay_transform_data (frame), schrolowdelay.c:1150-1200, with frame->iwt_frame on the
 * device (s16): `slices` (host, slices_bytes = slice_bytes_num * slices / slice_bytes_denom) receives what the reference
 * appends to frame->pack, base_index (host, one byte per slice; may be NULL) the chosen indices, *overruns (may be NULL)
 * the number of slices cut where the reference asserts.  The frame is not written (schro_hip_lowdelay_encode_batch's
 * first departure).  Copies back on the selected queue and waits for it. */
int schro_hip_encode_lowdelay_transform_data (const SchroHipFrame * iwt_frame, void *slices, size_t slices_bytes,
    const SchroHipLowDelayParams * params, uint8_t * base_index, int *overruns);

/* schro_encoder_encode_transform_data (frame) for params->is_noarith, schroencoder.c:3462-3483, with frame->quant_frame
 * on the device (schro_hipframe_quantise has run): the bytes the reference appends to frame->pack arrive in the HOST
 * buffer `out`, at most `capacity` of them; *bytes is what the picture takes.  quant_indices[k]: the quant index of every
 * record of component k in schro_hip_codeblock_layout's order, as schro_hipframe_quantise takes them.  subband_bits (or
 * NULL): frame->actual_subband_bits, [component][index]; false_zero (or NULL): the codeblocks and the sub-bands the s16
 * zero test called zero over non-zero values (schro_hip_noarith_encode_batch (a)).  Returns 0, or SCHRO_HIP_ENOMEM with
 * *bytes set when the picture takes more than `capacity` (schro_hip_noarith_encode_bound always suffices).  Copies back
 * on the selected queue and waits for it. */
int schro_hip_encode_transform_data_noarith (const SchroHipFrame * quant_frame, const SchroHipParams * params,
    const int *const quant_indices[3], void *out, size_t capacity, size_t *bytes,
    int subband_bits[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS], int false_zero[2]);

/* The motion data of a noarith picture, schroencoder.c:2505-2515 with params->is_noarith: motion->motion_vectors is the
 * HOST field of params->x_num_blocks * params->y_num_blocks records (no device frame comes with it, so the context is
 * an argument); the bytes the reference appends to frame->pack arrive in the HOST buffer `out`, at most `capacity` of
 * them; *bytes is what the picture takes, section_bytes (or NULL) the payload of each section, result (or NULL) the
 * whole SchroHipMotionEncodeResult.  Returns 0, or SCHRO_HIP_ENOMEM with *bytes set when the picture takes more than
 * `capacity` (schro_hip_motion_encode_bound always suffices).  Copies on the selected queue and waits for it. */
int schro_hip_encode_motion_data_noarith (SchroHipContext * ctx, const SchroHipMotion * motion, const SchroHipParams * params,
    void *out, size_t capacity, size_t *bytes, int section_bytes[SCHRO_HIP_MOTION_SECTIONS], SchroHipMotionEncodeResult * result);

/* The way back, schro_decoder_parse_block_data + schro_decoder_decode_block_data (schrodecoder.c:2531-2814) with
 * params->is_noarith: `length` HOST bytes at `data`, from a synchronised position, go up; motion->motion_vectors, the
 * HOST field of params->x_num_blocks * params->y_num_blocks records, is filled -- every byte of it --, and result (or
 * NULL) is the whole SchroHipMotionDecodeResult.  A length of 0 is allowed (data may be NULL then).  Copies on the
 * selected queue and waits for it. */
int schro_hip_decode_motion_data_noarith (SchroHipContext * ctx, const void *data, size_t length, const SchroHipParams * params,
    SchroHipMotion * motion, SchroHipMotionDecodeResult * result);

/* The same for an arithmetic-coded picture (schro_hip_motion_arith_decode_batch): refuses params->is_noarith; result (or
 * NULL) is the whole SchroHipMotionArithDecodeResult. */
int schro_hip_decode_motion_data_arith (SchroHipContext * ctx, const void *data, size_t length, const SchroHipParams * params,
    SchroHipMotion * motion, SchroHipMotionArithDecodeResult * result);

/* r05 -- the quantised hand-over behind the frame layer (VERDICT r04 "missing" 1): what a patched
 * schro_decoder_decode_subband (schrodecoder.c:3525-3640) leaves behind for one picture instead of a dense
 * coefficient frame.  Per component: the codeblock records in the decoder's order (their geometry from
 * schro_hip_codeblock_layout with the DEVICE transform frame's stride; src_offset / src_bytes / quant_index filled
 * in as schro_decoder_decode_codeblock goes, src_offset -1 for a zero codeblock, :3311-3322) and the quantised
 * values of its non-zero codeblocks, row-major and tight, 1 / 2 / 4 bytes each (src_offset counts from the
 * component's `values`).  INTEGRATION 3 shows the #ifdef HAVE_HIP branch. */
typedef struct {
  const SchroHipCodeblock *codeblocks[3];       /* HOST arrays (read during the call) */
  int ncodeblocks[3];
  const void *values[3];        /* values_on_device: device pointers (the host uploaded the picture's blob on the copy queue,
                                 * INTEGRATION 3a); else host pointers, copied by the call (pinned memory if the copy is to be asynchronous) */
  size_t values_bytes[3];
  int values_on_device;
} SchroHipQuantisedPicture;

/* transform_frame: the picture's DEVICE transform frame (s16 or s32), filled completely: zero codeblocks are zero-filled,
 * the others dequantised with the arithmetic of the decoder the picture takes (params->is_noarith on an s16 frame: the
 * 16-bit Orc program of the VLC path, schroorc.orc:1098-1219; else C int, schrodecoder.c:3072-3079), and for a picture
 * without references (params->num_refs == 0) the LL band of every component is DC-predicted (:3629-3636, :3219-3277).
 * What follows is schro_frame_inverse_iwt_transform_hip (frame, transform_frame, params) as before.  The launch
 * geometry is kept in a plan of the context's (schro_hip_dequant_plan_*), rebuilt when the picture geometry changes.
 * Enqueued on the selected queue; complete on return unless stage completion is off. */
int schro_hipframe_dequantise (SchroHipFrame * transform_frame, const SchroHipQuantisedPicture * quantised,
    SchroHipParams * params);

/* schro_decoder_parse_transform_data + schro_decoder_decode_transform_data (frame) for params->is_noarith
 * (schro_hip_noarith_decode_batch): `length` bytes of the picture's transform data, from a synchronised position on the
 * HOST, go up; transform_frame (a device frame, s16 or s32) is filled as schro_hipframe_dequantise leaves it, the LL bands
 * of an intra picture (params->num_refs == 0) DC-predicted.  *compat_quant_offset is the decoder instance's state: read,
 * and updated when the picture decodes.  *result is always filled when the call reaches the device; picture->error
 * (a header quant index above 60) returns SCHRO_HIP_EINVAL with the frame untouched.  Waits for the result. */
int schro_hipframe_decode_transform_data_noarith (SchroHipFrame * transform_frame, const uint8_t * host_data, size_t length,
    SchroHipParams * params, int *compat_quant_offset, SchroHipNoarithDecodeResult * result);

/* The same for an arithmetic-coded picture (schro_hip_arith_decode_batch): uploads, decodes, DC-predicts the LL bands of
 * an intra picture once picture->error is known to be 0, and waits.  params->is_noarith and params->is_lowdelay are
 * refused with SCHRO_HIP_EINVAL. */
int schro_hipframe_decode_transform_data_arith (SchroHipFrame * transform_frame, const uint8_t * host_data, size_t length,
    SchroHipParams * params, int *compat_quant_offset, SchroHipArithDecodeResult * result);

/* schro_upsampled_gpuframe_upsample (schrogpuframe.h:27) replacement:
 * dest (device, is_upsampled) <- half-pel images of src (device u8). */
int schro_upsampled_hipframe_upsample (SchroHipFrame * dest, SchroHipFrame * src);
/* the reference's one-argument form (schrogpuframe.h:29): `frame` is the upsampled device frame, its
 * integer-pel source the frame it keeps in virt_frame1 */
int schro_upsampled_hipframe_upsample_inplace (SchroHipFrame * frame);

/* schro_motion_render (motion, dest, addframe, add, output_frame) (schromotion.h:100, as
 * x_render_motion calls it, schrodecoder.c:1905-1935) replacement, same arguments.  add TRUE: the CPU path's
 * fused form -- `dest` (its s16 scratch frame) is not used and may be NULL.  add FALSE (r04): the prediction alone
 * into `dest`, a u8 device frame (schro_motion_render_cuda (motion, mc_tmp_frame), :1759), addframe and output_frame
 * NULL -- for schro_frame_inverse_iwt_transform_combine_hip; DC values outside [-128, 127] are an error there.  addframe:
 * device s16/s32 residual (picture->frame), or NULL for a zero_residual picture (nothing is added,
 * nothing is read: schrodecoder.c:1904-1906); output_frame: device u8.  motion->motion_vectors: the
 * host array, or a device copy of it.  Global motion is not
 * supported (the reference routes it to a different renderer, schromotion.c:113-118)
 * -> SCHRO_HIP_EUNSUPPORTED.
 * r06 -- add FALSE with an S16 device frame as `dest`: the literal contract of schro_motion_render_cuda (motion,
 * mc_tmp_frame) (schrocuda.h:13; schrodecoder.c:1742-1760, where mc_tmp_frame is an S16 frame of the transform's padded
 * size): dest receives the prediction - 128 in the reference's 16-bit arithmetic ((acc - 8160) >> 6,
 * orc_rrshift6_s16_ip_2d / _sub_s16_2d's d2) over the area the references cover; any weights, any DC values, never
 * SCHRO_HIP_ENEEDS_RESIDUAL.  schro_hipframe_add (picture->frame, mc_tmp_frame) and schro_hipframe_convert (output,
 * picture->frame) then finish the picture exactly as the HAVE_CUDA branch does (:1908-1910, :2011). */
int schro_motion_render_hip (SchroHipMotion * motion, SchroHipFrame * dest,
    SchroHipFrame * addframe, int add, SchroHipFrame * output_frame);

/* schro_gpuframe_add (dest, src) (schrogpuframe.h:18; call site schrodecoder.c:1908-1910) = schro_frame_add
 * (schroframe.c:1000-1029) on device frames: dest (S16) += src (S16, or U8 zero-extended) of the same chroma format,
 * 16-bit wrapping add over the components' common size.  Other depth pairs: SCHRO_HIP_EINVAL (the reference asserts). */
int schro_hipframe_add (SchroHipFrame * dest, SchroHipFrame * src);

/* schro_frame_subtract (dest, src) (schroframe.c:1062-1079) on device frames: dest (S16) -= src (S16, or U8 zero-extended) of
 * the same chroma format, 16-bit wrapping, over the components' common size -- the encoder's residual.  Other format pairs:
 * SCHRO_HIP_EINVAL (the reference asserts). */
int schro_hipframe_subtract (SchroHipFrame * dest, SchroHipFrame * src);

/* schro_encoder_quantise_subband over every sub-band of every component (the loop of schro_encoder_encode_subband's
 * callers, schroencoder.c:3789-3890) with frame->iwt_frame and frame->quant_frame on the device: both frames are device
 * frames of one domain, depth (s16 / s32) and chroma format.  The codeblocks, their order and their counts are
 * schro_hip_codeblock_layout's over params (iwt_luma_* / iwt_chroma_*, transform_depth, horiz_ / vert_codeblocks), the
 * stream's; quant_indices[c] holds one index per record of component c in that order (the values
 * schro_encoder_frame_get_quant_index returns).  A picture without references (params->num_refs == 0) is intra, and its
 * sub-band 0 is DC-predicted.  summary[c]: HOST arrays of as many entries, copied back on the selected queue -- complete
 * on return, or, when stage completion is off, once that queue has been waited for; allocate them with
 * schro_hip_host_alloc then: into pageable memory the copy holds the caller until it is done.  The records and the device
 * summaries -- a set per queue, so that pictures in flight on different queues do not share one -- are kept in a table of
 * the context's, rebuilt when the geometry changes. */
int schro_hipframe_quantise (SchroHipFrame * quant_frame, SchroHipFrame * iwt_frame, const SchroHipParams * params,
    const int *const quant_indices[3], SchroHipCodeblockSummary * const summary[3]);

/* schro_encoder_generate_subband_histograms (schroquantiser.c:618-637) with frame->iwt_frame on the device: what it
 * leaves in frame->subband_hists.  SchroHipHistogram is LAYOUT-IDENTICAL to SchroHistogram (schrohistogram.h:16-20), so
 * the reference's estimate and choice code (schro_histogram_estimate_entropy, schro_histogram_apply_table, ...) runs on
 * the result unchanged (on the host; schro_hip_quant_choose_batch is that code on the device, behind
 * schro_hip_histogram_batch).  hists: 3 * (1 + 3 * transform_depth) HOST entries, component-major, sub-band index minor;
 * bins[k] = counts * skip and n = sampled values * skip, skip = 1 << max (0, SCHRO_SUBBAND_SHIFT (position) - 1).  The
 * sub-band rectangles are schro_hip_codeblock_layout's with 1 x 1 codeblocks; sub-band 0 takes the DC-predict form when
 * params->num_refs == 0; a sub-band of no width or height gives an all-zero histogram.  overflow (may be NULL): as many
 * words, the samples of each sub-band whose bin index is >= 104, scaled by skip like the bins (see
 * SchroHipHistogramCounts: n = the bins' sum + overflow); the reference would have written past its array for them.
 * 840 bytes per sub-band cross the bus instead of the coefficient frame.  The integer counts are copied back on the
 * selected queue and scaled to doubles by the host once that copy has completed, so the call ALWAYS waits for the selected
 * queue (that queue only), whatever schro_hip_context_set_stage_completion says: hists and overflow are valid on
 * return.  The band records and the counts -- on the device and in pinned host memory, a set per queue -- are kept in a
 * table of the context's, rebuilt when the geometry changes. */
typedef struct {
  int n;
  double bins[SCHRO_HIP_HISTOGRAM_BINS];
} SchroHipHistogram;            /* layout-identical to SchroHistogram */
int schro_hipframe_subband_histograms (SchroHipFrame * iwt_frame, const SchroHipParams * params,
    SchroHipHistogram * hists, uint32_t * overflow /* may be NULL */);

/* schro_encoder_choose_quantisers (schroquantiser.c:288-316) for the engines rdo_bit_allocation, rdo_lambda, rdo_cbr and
 * constant_error with frame->iwt_frame on the device, SYNCHRONOUS: the histograms as above (is_intra and the DC form from
 * params->num_refs == 0), schro_hip_quant_choose_batch on their device counts, and the SchroHipQuantChoice in `result`
 * (HOST memory) on return: quant_index is frame->quant_indices, frame_lambda frame->frame_lambda; estimated_residual_bits
 * is the truncating int sum of chosen_entropy (:785-798).  schro_hip_quant_choose_tables comes first.  Refusals: those of
 * the two calls (the settings' after the histograms have run); waits for the selected queue whatever the stage setting. */
typedef struct {
  int is_noarith;               /* params->is_noarith */
  int engine;                   /* SCHRO_HIP_QUANT_ENGINE_* */
  double target;                /* the frame lambda, the bits, or the error */
  double subband_weight[SCHRO_HIP_NOARITH_MAX_SUBBANDS];
  double context_ratio[3][SCHRO_HIP_NOARITH_MAX_SUBBANDS];
  double subband0_lambda_scale, chroma_lambda_scale, diagonal_lambda_scale;
} SchroHipQuantChooseSettings;
int schro_encoder_choose_quantisers_hip (SchroHipFrame * iwt_frame, const SchroHipParams * params,
    const SchroHipQuantChooseSettings * settings, SchroHipQuantChoice * result);

/* schro_gpuframe_convert (schrogpuframe.h:20) replacement for the conversions the decode path
 * performs: s16/s32 -> u8 (+128, clamp, crop), u8 -> u8 copy, planar -> packed (YUYV, UYVY,
 * AYUV from u8; v210, v216, ARGB, AY64 from u8 / s16 / s32). */
int schro_hipframe_convert (SchroHipFrame * dest, SchroHipFrame * src);
/* The ENCODER-direction schro_frame_convert (schro_encoder_push_frame_full, schroencoder.c:1048-1058, and the intra
 * picture's convert into the transform frame, :2454) for two device frames of one domain: src a packed frame (YUYV, UYVY,
 * AYUV, v210, v216, AY64) or a planar one, dest a planar u8 / s16 / s32 frame -- unpack, depth, u8 chroma decimation,
 * crop or edge extension, as schro_hip_unpack_batch states and refuses them.  schro_hipframe_convert above keeps to the
 * decode path. */
int schro_hipframe_convert_input (SchroHipFrame * dest, SchroHipFrame * src);
/* An intra picture from the packed device frame the application handed over to the coefficients in iwt_frame (s16 / s32,
 * its components holding params->iwt_luma_* / iwt_chroma_*), picture_width x picture_height the video format's size:
 * schro_hip_unpack_iwt_batch.  Same coefficients as schro_hipframe_convert_input into a picture-sized frame of the
 * packed format's own depth, schro_hipframe_convert_input from that into iwt_frame, schro_hipframe_iwt_transform. */
int schro_hipframe_unpack_iwt_transform (SchroHipFrame * iwt_frame, SchroHipFrame * packed, const SchroHipParams * params,
    int picture_width, int picture_height);
/* schro_frame_shift_right (schroframe.c:1265-1293) on a device s16 / s32 frame */
int schro_hipframe_shift_right (SchroHipFrame * frame, int shift);

/* ---- picture statistics: average luma, squared error, SSIM, and the Gaussian low-pass under it ---------------
 *
 * The three measurements the reference's encoder takes of pictures this library keeps on the device:
 * schro_frame_calculate_average_luma (schro_encoder_analyse_picture, schroencoder.c:2252-2261), schro_frame_mean_squared_error
 * (schro_engine_get_scene_change_score, schroengine.c:304-345; enable_psnr, schroencoder.c:2728-2751) and schro_frame_ssim
 * (enable_ssim; schrossim.c:64-149), and schro_frame_filter_lowpass2 (schrofilter.c:516-814), which SSIM runs five times
 * and which is also the encoder's pre-filter `filtering = 2`.
 *
 * SUMS.  One job: the sum of plane `a` (u8: bytes_per_sample 1, s16: 2) and, when `b` is given (u8 against u8 only), the
 * sum of (a - b)^2.  Per sample this is orc_sum_u8 / orc_sum_s16 / orc_sum_square_diff_u8 (schroorc-dist.c:9361-9548); the
 * 16-bit mullw of the squared difference never loses a bit for u8 inputs (255^2 = 65025 < 65536).  The plane layer's sums
 * are EXACT 64-bit integers, accumulated in integers only (the same bits on every run), and stay in device memory:
 * result[0] the sum of a, result[1] the sum of squares (0 without b).  The call clears the two words and adds to them, all
 * on the selected queue; nothing is waited for.  Jobs of unlike size and depth mix freely in one call; two jobs must not
 * share a result. */
typedef struct {
  const void *a;                /* device */
  int a_stride;                 /* bytes */
  int bytes_per_sample;         /* 1: u8, 2: s16 */
  int width, height;
  const uint8_t *b;             /* device u8 plane, or NULL */
  int b_stride;
  int b_width, b_height;        /* must be width, height when b is given (schroanalysis.c:50-51) */
  int64_t *result;              /* device, 8-byte aligned, two words */
} SchroHipSumsJob;
int schro_hip_plane_sums_batch (SchroHipContext * ctx, const SchroHipSumsJob * jobs, int njobs);
/* host only: the refusals of schro_hip_plane_sums_batch without a context; no device pointer is dereferenced */
int schro_hip_plane_sums_check (const SchroHipSumsJob * jobs, int njobs);

/* LOW-PASS.  generate_coeff (schrofilter.c:666-689) on the host: the four doubles of one sigma. */
void schro_hip_lowpass2_coeff (double sigma, double coeff[4]);
/* schro_frame_component_filter_lowpass2_u8 / _s16 on one plane IN PLACE: every row forward then reverse with h_coeff, the
 * columns forward, the columns reverse with v_coeff, each pass rounded to the sample type before the next reads it, with
 * the reference's start states (s[0]; d[n - 1] after the forward pass; row 0 as the rows left it; the last row as the
 * forward column pass left it).  A step is x = c0 * s + c1 * i0 + c2 * i1 + c3 * i2 in IEEE double, left to right, four
 * rounded products and three rounded sums (no fused multiply-add), the stored sample rint (x).  Where rint (x) leaves the
 * sample type's range the reference's x86-64 build stores the low 8 / 16 bits of the value converted to int32; so does
 * this call, and it ADDS the number of such samples (of all four passes) to *out_of_range, which the caller clears.  For
 * sigma below about 0.7 the filter sharpens and this happens on real pictures (the chroma of a 4:2:0 picture at
 * filter_value 0.75); from sigma 0.75 up a 0 -> 255 step gives none.  Planes of unlike size, depth and coefficients mix in
 * one call; several planes may share one counter.  No two planes may share a byte: planes whose byte extents (first sample
 * to last) are apart pass, and so do windows of one buffer side by side -- equal strides, column ranges apart within the
 * stride --; any other two planes whose extents meet are refused. */
typedef struct {
  void *data;                   /* device; 2-byte aligned with an even stride for s16 */
  int stride;                   /* bytes */
  int bytes_per_sample;         /* 1: u8, 2: s16 */
  int width, height;
  double h_coeff[4], v_coeff[4];        /* finite */
  uint32_t *out_of_range;       /* device, 4-byte aligned; added to */
} SchroHipLowpass2Plane;
int schro_hip_lowpass2_batch (SchroHipContext * ctx, const SchroHipLowpass2Plane * planes, int nplanes);
int schro_hip_lowpass2_check (const SchroHipLowpass2Plane * planes, int nplanes);

/* SSIM.  What schro_frame_ssim reads, of the luma planes a and b (u8, one size): a_lowpass, b_lowpass the u8 low-pass at
 * sigma = width / 256.0 * 1.5; a_hipass = (a - 128) - a_lowpass, b_hipass likewise (s16: schro_frame_dup16 converts u8 to s16 with
 * the offset of orc_offsetconvert_s16_u8, so the values are -383 .. 127); the products ab, a^2, b^2 clamped to
 * [-32768, 32767] (schrossim.c:49-50; they reach 146689, the clamp bites), each low-passed as s16; then per pixel
 *   (2 mu_x mu_y + c1) (2 sigma_xy + c2) / ((mu_x^2 + mu_y^2 + c1) (sigma_x^2 + sigma_y^2 + c2)),
 * the integer terms in int, the rest in double without contraction: every pixel's value is the reference's bit for bit
 * and goes to `map` when one is given.  result->sum is their sum in a fixed order of this library's (rows of 8 within
 * columns of 256, a fixed tree, the tiles in raster order), the same bits on every run but NOT the reference's raster-order
 * accumulator's: two orders of adding the same n doubles differ by at most 2 (n - 1) 2^-53 sum |value|.  mssim = sum / (width * height) is the caller's (the
 * frame layer's).  out_of_range[k]: the count of schro_hip_lowpass2_batch for a_lowpass, b_lowpass, ab, a^2, b^2.
 * scratch: schro_hip_ssim_scratch_bytes (width, height) bytes of device memory, 16-byte aligned, the picture's own: what a
 * picture writes (scratch, result, map) may share no byte with anything the call reads or writes, of this picture or of
 * another (refused); a and b may be one plane, and pictures may share inputs. */
typedef struct {
  double sum;
  uint32_t out_of_range[5];
  uint32_t reserved;
} SchroHipSsimResult;
typedef struct {
  const uint8_t *a;             /* device */
  int a_stride;
  int width, height;
  const uint8_t *b;
  int b_stride;
  int b_width, b_height;        /* must be width, height */
  void *scratch;
  size_t scratch_bytes;
  SchroHipSsimResult *result;   /* device, 8-byte aligned */
  double *map;                  /* device, 8-byte aligned, or NULL */
  int map_stride;               /* bytes, a multiple of 8 */
} SchroHipSsimPicture;
size_t schro_hip_ssim_scratch_bytes (int width, int height);
int schro_hip_ssim_batch (SchroHipContext * ctx, const SchroHipSsimPicture * pictures, int npictures);
int schro_hip_ssim_check (const SchroHipSsimPicture * pictures, int npictures);
/* The tile and chunk lengths of the kernels above, for tests and tools that place planes around them: values[0 .. 7] =
 * bytes and rows of a sums tile; rows of a row-pass workgroup, columns of a chunk it stages, columns of a column-pass
 * workgroup, rows a column-pass lane loads at a time; columns and rows of an SSIM tile. */
#define SCHRO_HIP_PICTURE_STATS_GEOMETRY 8
void schro_hip_picture_stats_geometry (int values[SCHRO_HIP_PICTURE_STATS_GEOMETRY]);

/* The frame layer, all synchronous, on device frames.
 * schro_frame_calculate_average_luma (schroframe.c:1647-1680) of a u8 or s16 frame: the reference accumulates in an
 * `int`, which a u8 plane of more than 8.42 M bright samples wraps (DCI 4K at level 255); this call returns the WRAPPED
 * value the reference's build returns -- (double) (int32) sum / (width * height) --, the plane layer above always has the
 * exact sum. */
int schro_hipframe_calculate_average_luma (SchroHipFrame * frame, double *out);
/* schro_frame_mean_squared_error (schroanalysis.c:44-84) of two u8 frames of one size and chroma format: the reference adds
 * per-row int32 sums as doubles, exact below 2^53, so the device's integer sum converted once is the same double. */
int schro_hipframe_mean_squared_error (SchroHipFrame * a, SchroHipFrame * b, double mse[3]);
/* schro_frame_ssim: sum / (width * height) of schro_hip_ssim_batch over the luma planes of two u8 frames */
int schro_hipframe_ssim (SchroHipFrame * a, SchroHipFrame * b, double *mssim);
/* schro_frame_filter_lowpass2 (schrofilter.c:784-814) of a u8 or s16 frame in place, the chroma sigmas divided by 1 <<
 * h_shift and 1 << v_shift of the format (:790-791); the out-of-range counts are dropped */
int schro_hipframe_filter_lowpass2 (SchroHipFrame * frame, double sigma);
/* schroengine.c:327-336 on the coarsest pyramid levels of a picture (frame1) and its predecessor (frame2): luma =
 * average_luma - 16; the score is mse[0] / (luma * luma) when luma > 0.01, else 1.0 (then nothing is launched) */
int schro_engine_get_scene_change_score_hip (SchroHipFrame * frame1, SchroHipFrame * frame2, double average_luma, double *score);

/* diagnostics: with SCHRO_HIP_OBMC_STAMPS set, the row / staged OBMC kernels record cycle stamps
 * per phase and workgroup; this prints their medians to stderr (scratch runs only) */
void schro_hip_obmc_stamps_dump (void);

/* ---- several devices behind one decode loop -----------------------------
 *
 * One exec-domain thread per device, each with its own context -- the reference's
 * schro_async_add_exec_domain thread (schroasync-pthread.c:362-390), N times -- and the
 * device-affinity rule the reference's scheduler lacks (schro_decoder_async_schedule,
 * schrodecoder.c:1546-1682; schro_picture_new :332-400): a picture runs on the device that
 * holds its first reference, so a reference chain (closed GOP) never leaves its device; a
 * picture without references starts a chain on the least loaded device (ties: the device holding the fewest live references).  A device runs its
 * pictures in submission (= coded) order, which puts references before their dependents.
 * `func` is the picture's pixel path -- the stage calls of this header on `ctx` -- and runs on
 * that device's thread; no collective, no peer traffic unless a picture predicts across two
 * chains (then *foreign_ref names the reference that lives elsewhere, the picture waits for
 * it, and moving that frame is the caller's: one u8 picture over xGMI). */
typedef struct SchroHipScheduler SchroHipScheduler;
typedef int (*SchroHipPictureFunc) (SchroHipContext * ctx, int device_index, void *priv);

/* n_devices 0: every visible device.  _virtual: threads and affinity without devices (ctx is
 * NULL in the callbacks): the host logic under test on a machine without GPUs. */
SchroHipScheduler *schro_hip_scheduler_new (int n_devices);
SchroHipScheduler *schro_hip_scheduler_new_virtual (int n_devices);
/* an explicit device list; a device may appear more than once (two exec-domain threads and contexts
 * on one device: how a box with one GPU exercises the cross-device paths) */
SchroHipScheduler *schro_hip_scheduler_new_on (const int *devices, int n_devices);
/* waits for everything submitted, stops the threads, frees the contexts */
void schro_hip_scheduler_free (SchroHipScheduler * sched);
int schro_hip_scheduler_n_devices (SchroHipScheduler * sched);
SchroHipContext *schro_hip_scheduler_context (SchroHipScheduler * sched, int device_index);
/* returns the device index the picture was given (< 0: error).  refs: the picture numbers it
 * predicts from (0 .. 2), each submitted earlier with is_ref != 0. */
int schro_hip_scheduler_submit (SchroHipScheduler * sched, int picture_number, const int *refs, int n_refs,
    int is_ref, SchroHipPictureFunc func, void *priv, int *foreign_ref);
/* A reference picture leaves the reference queue (schro_decoder_reference_retire,
 * schrodecoder.c:1302 -- at PARSE time, possibly before pictures that predict from it, or the
 * reference itself, have run): later submits no longer find the number; pictures already submitted
 * keep what they resolved, and the reference's frames go when the last of them has finished. */
int schro_hip_scheduler_retire (SchroHipScheduler * sched, int picture_number);
/* r03 -- references move, not just wait.  The function of a reference picture publishes the device
 * frame its dependents read (the upsampled frame when mv_precision > 0, else the plain one); the
 * scheduler keeps a reference on it.  Before a picture with a reference on ANOTHER device runs, that
 * frame is copied to the picture's device (schro_hip_frame_copy_to: one hipMemcpyPeerAsync per
 * component; the owner's device work is complete by then) and cached there for later dependents;
 * schro_hip_scheduler_reference_frame, called by a picture's function, gives the frame of one of ITS
 * references on ITS device -- the published frame or the copy (NULL: nothing was published: the
 * foreign_ref of submit names what the caller has to move itself).  On virtual devices the
 * "frames" are opaque pointers that are handed through. */
int schro_hip_scheduler_publish_reference (SchroHipScheduler * sched, int device_index, void *frame);
void *schro_hip_scheduler_reference_frame (SchroHipScheduler * sched, int device_index, int picture_number);
long schro_hip_scheduler_moves (SchroHipScheduler * sched);       /* frames copied between devices so far */
/* r04: nothing on the path drains a device.  A reference picture is complete when an event stands behind
 * the work its function enqueued; pictures of the same device follow it in the in-order KERNEL queues (r05:
 * both of them wait for that event, and every picture function starts with queue 0 selected; what a function
 * puts on the COPY queues it orders itself with marks), a picture
 * on another device waits for the event on its copy queue and copies asynchronously (TODO-CUDA:5-7) -- the
 * scheduler waits for nothing itself, and the peer copy does not hold its caller either (measured: 22 us in the
 * call behind an unfired event, two contexts on one device, profiles/r05_peer_copy_hip_trace.txt; unlike copies from /
 * to pinned host memory; a copy between two real devices is unmeasured).
 * r05: a frame the scheduler lets go of (a retired reference, its copies on other devices) is released only
 * when the kernel queues of its device have passed that point -- kernels of dependents may still read it.
 * A reference whose function returned an error is marked failed: its dependents -- and theirs -- do not
 * run, they finish with SCHRO_HIP_ESKIPPED (the reference decoder skips such pictures: picture->error,
 * schrodecoder.c:1308-1311, :1399-1418); schro_hip_scheduler_wait still reports the first real error. */
long schro_hip_scheduler_skipped (SchroHipScheduler * sched);     /* pictures skipped so far */
/* most reference pictures of ONE device whose device work was still running when the next one had been enqueued */
int schro_hip_scheduler_refs_in_flight_max (SchroHipScheduler * sched);
/* waits until every submitted picture has run; returns the first non-zero result of a func */
int schro_hip_scheduler_wait (SchroHipScheduler * sched);

#ifdef __cplusplus
}
#endif
#endif
