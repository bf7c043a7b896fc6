// plane_quant_choose.cpp -- plane layer: the quantiser choice (quant_choose.hip): schro_hip_quant_choose_tables keeps the
// encoder's tables on the device, schro_hip_quant_choose_batch turns the pictures of a call into the records of one
// estimate and one choice launch, schro_hip_quant_choose_check holds its refusals without a context.

#include "schro_hip_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace schro;

namespace schro {

static int
quant_choose_check_run (const SchroHipQuantChoosePicture * pictures, int npictures, bool have_bit_tables)
{
  SCHRO_HIP_REQUIRE (pictures && npictures > 0, "quant_choose: bad arguments");
  for (int p = 0; p < npictures; p++) {
    const SchroHipQuantChoosePicture & pic = pictures[p];
    SCHRO_HIP_REQUIRE (pic.transform_depth >= 0 && pic.transform_depth <= 6, "quant_choose: picture %d: a transform_depth of %d (0 .. 6)", p,
        pic.transform_depth);
    SCHRO_HIP_REQUIRE ((pic.is_intra == 0 || pic.is_intra == 1) && (pic.is_noarith == 0 || pic.is_noarith == 1),
        "quant_choose: picture %d: is_intra %d, is_noarith %d (0 or 1 each)", p, pic.is_intra, pic.is_noarith);
    SCHRO_HIP_REQUIRE (pic.engine == SCHRO_HIP_QUANT_ENGINE_LAMBDA || pic.engine == SCHRO_HIP_QUANT_ENGINE_BIT_ALLOCATION
        || pic.engine == SCHRO_HIP_QUANT_ENGINE_CONSTANT_ERROR, "quant_choose: picture %d: engine %d is unknown", p, pic.engine);
    SCHRO_HIP_REQUIRE (pic.is_noarith || have_bit_tables,
        "quant_choose: picture %d: is_noarith 0 needs the one-bits and zero-bits tables (schro_hip_quant_choose_tables)", p);
    const int nb = 1 + 3 * pic.transform_depth;
    for (int i = 0; i < nb; i++) {
      SCHRO_HIP_REQUIRE (pic.skip[i] >= 1 && pic.skip[i] <= 1024 && (pic.skip[i] & (pic.skip[i] - 1)) == 0,
          "quant_choose: picture %d: skip[%d] is %d (a power of two, 1 .. 1024)", p, i, pic.skip[i]);
      SCHRO_HIP_REQUIRE (std::isfinite (pic.subband_weight[i]) && pic.subband_weight[i] > 0,
          "quant_choose: picture %d: subband_weight[%d] is %g (finite and positive)", p, i, pic.subband_weight[i]);
      for (int c = 0; c < 3; c++)
        SCHRO_HIP_REQUIRE (std::isfinite (pic.context_ratio[c][i]), "quant_choose: picture %d: context_ratio[%d][%d] is %g (finite)", p, c,
            i, pic.context_ratio[c][i]);
    }
    SCHRO_HIP_REQUIRE (std::isfinite (pic.subband0_lambda_scale), "quant_choose: picture %d: subband0_lambda_scale is %g (finite)", p,
        pic.subband0_lambda_scale);
    SCHRO_HIP_REQUIRE (std::isfinite (pic.chroma_lambda_scale), "quant_choose: picture %d: chroma_lambda_scale is %g (finite)", p,
        pic.chroma_lambda_scale);
    SCHRO_HIP_REQUIRE (std::isfinite (pic.diagonal_lambda_scale), "quant_choose: picture %d: diagonal_lambda_scale is %g (finite)", p,
        pic.diagonal_lambda_scale);
    SCHRO_HIP_REQUIRE (std::isfinite (pic.target), "quant_choose: picture %d: target is %g (finite)", p, pic.target);
    for (int c = 0; c < 3; c++)
      SCHRO_HIP_REQUIRE (pic.counts[c] && (uintptr_t) pic.counts[c] % sizeof (uint32_t) == 0,
          "quant_choose: picture %d: counts[%d] is NULL or not 4-byte aligned", p, c);
    SCHRO_HIP_REQUIRE (pic.result && (uintptr_t) pic.result % sizeof (double) == 0, "quant_choose: picture %d: result is NULL or not 8-byte aligned", p);
    SCHRO_HIP_REQUIRE ((uintptr_t) pic.est_entropy % sizeof (double) == 0 && (uintptr_t) pic.est_error % sizeof (double) == 0,
        "quant_choose: picture %d: est_entropy / est_error not 8-byte aligned", p);
  }
  return 0;
}

void
quant_choose_tables_free (SchroHipContext * ctx)
{
  if (!ctx->qc_tables && !ctx->qc_frame_choice)
    return;
  for (int q = 0; q < SchroHipContext::kQueues; q++)    // launches that still read the tables or write the records
    if (ctx->streams[q])
      (void) hipStreamSynchronize (ctx->streams[q]);
  if (ctx->qc_tables)
    (void) hipFree (ctx->qc_tables);
  if (ctx->qc_frame_choice)
    (void) hipFree (ctx->qc_frame_choice);
  ctx->qc_tables = nullptr;
  ctx->qc_frame_choice = nullptr;
  ctx->qc_have_bits = false;
}

}                               // namespace schro

extern "C" {

int
schro_hip_quant_choose_tables (SchroHipContext * ctx, const double *error, const double *onebits, const double *zerobits)
{
  SCHRO_HIP_REQUIRE (ctx && error, "quant_choose_tables: a context and the error table are needed");
  SCHRO_HIP_REQUIRE ((onebits != nullptr) == (zerobits != nullptr), "quant_choose_tables: onebits and zerobits come together or not at all");
  (void) hipSetDevice (ctx->device);
  // [60][104] as the encoder holds them -> [104][60]
  std::vector < double >t ((size_t) 3 * kQcTableDoubles, 0.0);
  const double *src[3] = { error, onebits, zerobits };
  for (int k = 0; k < 3; k++)
    if (src[k])
      for (int j = 0; j < kQcIndices; j++)
        for (int i = 0; i < SCHRO_HIP_HISTOGRAM_BINS; i++)
          t[(size_t) k * kQcTableDoubles + (size_t) i * kQcIndices + j] = src[k][j * SCHRO_HIP_HISTOGRAM_BINS + i];
  for (int q = 0; q < SchroHipContext::kQueues; q++)    // launches that still read the tables being replaced
    if (ctx->streams[q])
      SCHRO_HIP_CHECK (hipStreamSynchronize (ctx->streams[q]));
  if (!ctx->qc_tables)
    SCHRO_HIP_CHECK (hipMalloc (&ctx->qc_tables, t.size () * sizeof (double)));
  SCHRO_HIP_CHECK (hipMemcpy (ctx->qc_tables, t.data (), t.size () * sizeof (double), hipMemcpyHostToDevice));
  ctx->qc_have_bits = onebits != nullptr;
  return 0;
}

int
schro_hip_quant_choose_check (const SchroHipQuantChoosePicture * pictures, int npictures, int have_bit_tables)
{
  return quant_choose_check_run (pictures, npictures, have_bit_tables != 0);
}

int
schro_hip_quant_choose_batch (SchroHipContext * ctx, const SchroHipQuantChoosePicture * pictures, int npictures)
{
  SCHRO_HIP_REQUIRE (ctx, "quant_choose_batch: bad arguments");
  SCHRO_HIP_REQUIRE (ctx->qc_tables, "quant_choose_batch: no tables (schro_hip_quant_choose_tables comes first)");
  int r = quant_choose_check_run (pictures, npictures, ctx->qc_have_bits);
  if (r)
    return r;
  SCHRO_HIP_REQUIRE (npictures <= 65535, "quant_choose_batch: %d pictures (at most 65535 in a call)", npictures);
  (void) hipSetDevice (ctx->device);
  std::vector < QcPicture > recs ((size_t) npictures);
  memset (recs.data (), 0, sizeof (QcPicture) * recs.size ());
  for (int p = 0; p < npictures; p++) {
    const SchroHipQuantChoosePicture & pic = pictures[p];
    QcPicture & rec = recs[p];
    for (int c = 0; c < 3; c++)
      rec.counts[c] = (const uint32_t *) pic.counts[c];
    rec.result = pic.result;
    rec.est_entropy = pic.est_entropy;
    rec.est_error = pic.est_error;
    const int nb = 1 + 3 * pic.transform_depth;
    for (int i = 0; i < kQcBands; i++) {
      // (entries past the depth are never read; a neutral value keeps the table's bytes a function of what is)
      rec.weight[i] = i < nb ? pic.subband_weight[i] : 1.0;
      rec.skip[i] = i < nb ? pic.skip[i] : 1;
      for (int c = 0; c < 3; c++)
        rec.ratio[c][i] = i < nb ? pic.context_ratio[c][i] : 1.0;
    }
    rec.scale[0] = pic.subband0_lambda_scale;
    rec.scale[1] = pic.chroma_lambda_scale;
    rec.scale[2] = pic.diagonal_lambda_scale;
    rec.target = pic.target;
    rec.depth = pic.transform_depth;
    rec.noarith = pic.is_noarith;
    rec.engine = pic.engine;
  }
  r = ensure_scratch (ctx, (size_t) npictures * 2 * kQcEstimates * sizeof (double));
  if (r)
    return r;
  const size_t bytes = sizeof (QcPicture) * recs.size ();
  void *d_pics;
  r = bytes <= SchroHipContext::kArgSlotBytes ? push_args (ctx, recs.data (), bytes, &d_pics) : push_big_table (ctx, recs.data (), bytes, &d_pics);
  if (r)
    return r;
  return launch_quant_choose (ctx->stream, (const QcPicture *) d_pics, npictures, ctx->qc_tables, ctx->qc_have_bits ? 1 : 0,
      (double *) ctx->scratch_ref ());
}

}                               // extern "C"
