// plane_lowdelay_enc.cpp -- plane layer: VC-2 low-delay slices written on the device (lowdelay_enc.hip).

#include "schro_hip_internal.h"

#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

extern "C" {

int
schro_hip_lowdelay_encode_batch (SchroHipContext * ctx, const SchroHipLowDelayEncodePicture * pictures, int npictures,
    const SchroHipLowDelayParams * params, int bytes_per_sample)
{
  SCHRO_HIP_REQUIRE (ctx && pictures && params && npictures > 0 && npictures <= kMaxJobs,
      "lowdelay_encode_batch: bad arguments");
  SCHRO_HIP_REQUIRE (bytes_per_sample != 4, "lowdelay_encode_batch: s32 slices are not encoded (the reference's encoder is s16)");
  SCHRO_HIP_REQUIRE (bytes_per_sample == 2, "lowdelay_encode_batch: bytes_per_sample must be 2");
  const SchroHipLowDelayParams & lp = *params;
  const int depth = lp.transform_depth;
  SCHRO_HIP_REQUIRE (depth >= 0 && depth <= 6, "lowdelay_encode_batch: transform_depth %d", depth);
  SCHRO_HIP_REQUIRE (lp.iwt_luma_width > 0 && lp.iwt_luma_height > 0 && lp.iwt_chroma_width > 0
      && lp.iwt_chroma_height > 0 && ((lp.iwt_luma_width | lp.iwt_luma_height | lp.iwt_chroma_width
              | lp.iwt_chroma_height) & ((1 << depth) - 1)) == 0 && lp.iwt_luma_width < (1 << 15) && lp.iwt_luma_height < (1 << 15)
      && lp.iwt_chroma_width < (1 << 15) && lp.iwt_chroma_height < (1 << 15),
      "lowdelay_encode_batch: iwt sizes must be positive multiples of 2^depth below 32768");
  SCHRO_HIP_REQUIRE (lp.n_horiz_slices > 0 && lp.n_vert_slices > 0 && lp.n_horiz_slices < (1 << 15) && lp.n_vert_slices < (1 << 15)
      && (int64_t) lp.n_horiz_slices * lp.n_vert_slices < (1 << 24), "lowdelay_encode_batch: bad slice counts");
  SCHRO_HIP_REQUIRE (lp.slice_bytes_denom > 0, "lowdelay_encode_batch: slice_bytes_denom %d", lp.slice_bytes_denom);
  SCHRO_HIP_REQUIRE (lp.slice_bytes_num >= lp.slice_bytes_denom, "lowdelay_encode_batch: slice_bytes %d / %d",
      lp.slice_bytes_num, lp.slice_bytes_denom);
  // the reference's reconstructed frame is the luma LL size in the frame's chroma format (schrolowdelay.c:1164-1166) and
  // its chroma LL rectangles are cut from THAT (:1015-1032): the same rectangles as the band's only where the sizes agree
  const int llw = lp.iwt_luma_width >> depth, llh = lp.iwt_luma_height >> depth;
  const int lcw = lp.iwt_chroma_width >> depth, lch = lp.iwt_chroma_height >> depth;
  const int hs = lp.iwt_chroma_width < lp.iwt_luma_width, vs = lp.iwt_chroma_height < lp.iwt_luma_height;
  SCHRO_HIP_REQUIRE (((llw + hs) >> hs) == lcw && ((llh + vs) >> vs) == lch,
      "lowdelay_encode_batch: chroma LL band %d x %d, the luma LL band %d x %d in the chroma format is %d x %d: the "
      "reference's rectangles diverge", lcw, lch, llw, llh, (llw + hs) >> hs, (llh + vs) >> vs);
  // the kernels index the reconstructed LL bands and a thread's LL samples with int: both stay far below 2^31
  const int64_t ll_samples = (int64_t) llw * llh + 2 * (int64_t) lcw * lch;
  SCHRO_HIP_REQUIRE (ll_samples <= ((int64_t) 1 << 28),
      "lowdelay_encode_batch: transform_depth %d leaves LL bands of %lld samples, more than 2^28", depth, (long long) ll_samples);
  const int64_t ll_slice = (int64_t) div_up (llw, lp.n_horiz_slices) * div_up (llh, lp.n_vert_slices)
      + 2 * (int64_t) div_up (lcw, lp.n_horiz_slices) * div_up (lch, lp.n_vert_slices);
  SCHRO_HIP_REQUIRE (ll_slice <= (1 << 20),
      "lowdelay_encode_batch: n_horiz_slices %d x n_vert_slices %d leave LL rectangles of %lld samples per slice, more than 2^20",
      lp.n_horiz_slices, lp.n_vert_slices, (long long) ll_slice);
  const int64_t nslices = (int64_t) lp.n_horiz_slices * lp.n_vert_slices;
  const int64_t need = ((int64_t) lp.slice_bytes_num * nslices) / lp.slice_bytes_denom;
  SCHRO_HIP_REQUIRE (need < ((int64_t) 1 << 28), "lowdelay_encode_batch: %lld bytes of slices per picture", (long long) need);
  for (int p = 0; p < npictures; p++) {
    const SchroHipLowDelayEncodePicture & pic = pictures[p];
    SCHRO_HIP_REQUIRE (pic.slices, "lowdelay_encode_batch: picture %d: slices is NULL", p);
    SCHRO_HIP_REQUIRE ((int64_t) pic.slices_bytes == need, "lowdelay_encode_batch: picture %d: slices_bytes %zu, the slices take %lld",
        p, pic.slices_bytes, (long long) need);
    SCHRO_HIP_REQUIRE (pic.base_index, "lowdelay_encode_batch: picture %d: base_index is NULL", p);
    SCHRO_HIP_REQUIRE (pic.overruns && (uintptr_t) pic.overruns % 4 == 0, "lowdelay_encode_batch: picture %d: overruns is NULL or unaligned", p);
    for (int k = 0; k < 3; k++) {
      const int w = k ? lp.iwt_chroma_width : lp.iwt_luma_width;
      SCHRO_HIP_REQUIRE (pic.comp[k] && (uintptr_t) pic.comp[k] % 2 == 0, "lowdelay_encode_batch: picture %d: comp[%d] is NULL or odd", p, k);
      SCHRO_HIP_REQUIRE (pic.stride[k] >= w * 2 && pic.stride[k] % 2 == 0,
          "lowdelay_encode_batch: picture %d: stride[%d] %d for %d samples of 2 bytes", p, k, pic.stride[k], w);
    }
  }
  (void) hipSetDevice (ctx->device);

  SliceParams P;
  memset (&P, 0, sizeof (P));
  P.depth = depth;
  P.iwt_lw = lp.iwt_luma_width;
  P.iwt_lh = lp.iwt_luma_height;
  P.iwt_cw = lp.iwt_chroma_width;
  P.iwt_ch = lp.iwt_chroma_height;
  P.nh = lp.n_horiz_slices;
  P.nv = lp.n_vert_slices;
  P.n_bytes = lp.slice_bytes_num / lp.slice_bytes_denom;
  P.remainder = lp.slice_bytes_num % lp.slice_bytes_denom;
  P.denom = lp.slice_bytes_denom;
  for (int i = 0; i < 1 + 3 * depth; i++)
    P.quant_matrix[i] = lp.quant_matrix[i];

  // what a thread of the serial launch keeps: its LL samples, the reconstructed row above and column to the left of each
  // component, and the row it is reconstructing -- sized for the largest rectangle of the picture (at most 2^20 samples
  // and three rows and columns of at most 2^15: per_thread * threads, the largest index, is below 2^29)
  EncChooseLayout L;
  memset (&L, 0, sizeof (L));
  int at = 0, bw_max = 0;
  for (int c = 0; c < 3; c++) {
    const int bw = div_up (c ? lcw : llw, P.nh), bh = div_up (c ? lch : llh, P.nv);
    L.coef[c] = at;
    at += bw * bh;
    L.top[c] = at;
    at += bw + 1;
    L.left[c] = at;
    at += bh;
    bw_max = std::max (bw_max, bw);
  }
  L.row = at;
  at += bw_max;
  L.per_thread = at;
  const int diag = std::min (P.nh, P.nv);
  const size_t kLds = 48u << 10;
  L.threads = std::min (1024, div_up (diag, 64) * 64);
  if ((size_t) L.per_thread * 2 * 64 <= kLds) {
    L.threads = std::min (L.threads, (int) (kLds / ((size_t) L.per_thread * 2)) / 64 * 64);
    L.in_lds = 1;
    L.lds_bytes = L.per_thread * 2 * L.threads;
  } else {
    L.threads = std::min (L.threads, 256);
  }
  L.recon_off[0] = 0;
  L.recon_off[1] = llw * llh;
  L.recon_off[2] = llw * llh + lcw * lch;

  // scratch of the selected queue: the estimate's table, the reconstructed LL bands, the serial launch's spill
  auto round16 = [] (size_t n) { return (n + 15) & ~(size_t) 15; };
  const size_t est_bytes = round16 ((size_t) nslices * 130 * sizeof (uint32_t));
  const size_t recon_bytes = round16 (((size_t) llw * llh + 2 * (size_t) lcw * lch) * 2);
  const size_t work_bytes = L.in_lds ? 0 : round16 ((size_t) L.per_thread * 2 * L.threads);
  const size_t per_picture = est_bytes + recon_bytes + work_bytes;
  int r = ensure_scratch (ctx, per_picture * (size_t) npictures);
  if (r)
    return r;
  char *scratch = (char *) ctx->scratch_ref ();

  std::vector < EncJob > jobs (npictures);
  for (int p = 0; p < npictures; p++) {
    const SchroHipLowDelayEncodePicture & pic = pictures[p];
    EncJob & j = jobs[p];
    memset (&j, 0, sizeof (j));
    for (int k = 0; k < 3; k++) {
      j.comp[k] = pic.comp[k];
      j.stride[k] = pic.stride[k];
    }
    j.out = pic.slices;
    j.index = pic.base_index;
    j.overrun = pic.overruns;
    char *mine = scratch + per_picture * (size_t) p;
    j.est = (uint32_t *) mine;
    j.recon = (int16_t *) (mine + est_bytes);
    j.work = (int16_t *) (mine + est_bytes + recon_bytes);
  }
  void *d_jobs;
  r = push_args (ctx, jobs.data (), sizeof (EncJob) * npictures, &d_jobs);
  if (r)
    return r;
  // (A/B runs, scripts/lowdelay_encode_ab.py: one launch at a time on the tables the call before left)
  const char *env = SCHRO_ENV ("SCHRO_HIP_LDENC_STAGES");
  const int stages = env && atoi (env) > 0 ? atoi (env) & 7 : 7;
  if (stages & 4)
    for (int p = 0; p < npictures; p++)
      SCHRO_HIP_CHECK (hipMemsetAsync (pictures[p].overruns, 0, sizeof (uint32_t), ctx->stream));
  // (no profile class: SCHRO_HIP_KERNEL_CLASSES is what it was; schro_hip_timer_begin / _end time the call)
  return launch_lowdelay_encode (ctx->stream, (const EncJob *) d_jobs, npictures, P, L, stages);
}

}                               // extern "C"
