// quant_choose_walk.cpp -- the host code of the quantiser choice (plane_quant_choose.cpp) and of the two consumers that
// take their indices from the device (schro_hip_quantise_chosen_batch in plane_quant.cpp,
// schro_hip_noarith_encode_chosen_batch / _check in plane_noarith_enc.cpp) walked under AddressSanitizer +
// UndefinedBehaviorSanitizer: a plain C++ program with its own main, linked with the objects of the library's
// device-free sanitizer build (make -C schroedinger_amd/csrc dry_asan).  Launches are dropped there, so what runs is the
// table transposition, every refusal, the record and run tables, the scratch arithmetic (small, large, small) and the
// table uploads.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "quant_choose_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

static void *
take (SchroHipContext * ctx, size_t bytes)
{
  void *m = schro_hip_domain_alloc (ctx, bytes);
  if (!m) {
    fprintf (stderr, "quant_choose_walk: no memory: %s\n", schro_hip_last_error ());
    exit (2);
  }
  return m;
}

static SchroHipQuantChoosePicture
choose_picture (SchroHipContext * ctx, int depth, int engine, int noarith, std::vector < void *>&owned)
{
  SchroHipQuantChoosePicture p;
  memset (&p, 0, sizeof (p));
  const int nb = 1 + 3 * depth;
  for (int c = 0; c < 3; c++) {
    // exactly the entries the depth needs: a read past them is the sanitizer's to find
    p.counts[c] = (const SchroHipHistogramCounts *) take (ctx, sizeof (SchroHipHistogramCounts) * nb);
    owned.push_back ((void *) p.counts[c]);
  }
  for (int i = 0; i < nb; i++) {
    p.skip[i] = 1 << (i % 6);
    p.subband_weight[i] = 1.0 + i;
    for (int c = 0; c < 3; c++)
      p.context_ratio[c][i] = 1.0;
  }
  p.transform_depth = depth;
  p.is_intra = depth & 1;
  p.is_noarith = noarith;
  p.engine = engine;
  p.subband0_lambda_scale = 10;
  p.chroma_lambda_scale = 0.1;
  p.diagonal_lambda_scale = 0.5;
  p.target = 1000;
  p.result = (SchroHipQuantChoice *) take (ctx, sizeof (SchroHipQuantChoice));
  owned.push_back (p.result);
  return p;
}

static bool
refused (int r, const char *fragment)
{
  return r == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), fragment) != nullptr;
}

int
main ()
{
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "quant_choose_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
    return 2;
  }
  std::vector < void *>owned;
  std::vector < double >error (60 * 104), ones (60 * 104, 1.5), zeros (60 * 104, 2.5);
  for (size_t k = 0; k < error.size (); k++)
    error[k] = (double) k;

  // ---- the choice: no tables, the error table alone, all three, replaced
  SchroHipQuantChoosePicture one = choose_picture (ctx, 2, SCHRO_HIP_QUANT_ENGINE_BIT_ALLOCATION, 1, owned);
  EXPECT (refused (schro_hip_quant_choose_batch (ctx, &one, 1), "no tables"), "a call without tables was not refused");
  EXPECT (refused (schro_hip_quant_choose_tables (ctx, error.data (), ones.data (), nullptr), "come together"), "one bit table alone");
  EXPECT (schro_hip_quant_choose_tables (ctx, error.data (), nullptr, nullptr) == 0, "tables (error alone)");
  EXPECT (schro_hip_quant_choose_batch (ctx, &one, 1) == 0, "one noarith picture");
  SchroHipQuantChoosePicture arith = choose_picture (ctx, 1, SCHRO_HIP_QUANT_ENGINE_LAMBDA, 0, owned);
  EXPECT (refused (schro_hip_quant_choose_batch (ctx, &arith, 1), "needs the one-bits"), "arith form without bit tables");
  EXPECT (schro_hip_quant_choose_tables (ctx, error.data (), ones.data (), zeros.data ()) == 0, "tables (all three)");
  EXPECT (schro_hip_quant_choose_batch (ctx, &arith, 1) == 0, "one arith picture");

  // ---- the refusals of the check, each on the second picture of two
  struct Bad {
    const char *fragment;
    void (*make) (SchroHipQuantChoosePicture &);
  };
  const Bad bads[] = {
    {"picture 1: a transform_depth of 7",[](SchroHipQuantChoosePicture & p) { p.transform_depth = 7; }},
    {"picture 1: skip[3] is 6",[](SchroHipQuantChoosePicture & p) { p.skip[3] = 6; }},
    {"picture 1: skip[0] is 2048",[](SchroHipQuantChoosePicture & p) { p.skip[0] = 2048; }},
    {"picture 1: subband_weight[2] is 0",[](SchroHipQuantChoosePicture & p) { p.subband_weight[2] = 0; }},
    {"picture 1: subband_weight[1] is nan",[](SchroHipQuantChoosePicture & p) { p.subband_weight[1] = NAN; }},
    {"picture 1: context_ratio[2][6] is inf",[](SchroHipQuantChoosePicture & p) { p.context_ratio[2][6] = INFINITY; }},
    {"picture 1: chroma_lambda_scale is nan",[](SchroHipQuantChoosePicture & p) { p.chroma_lambda_scale = NAN; }},
    {"picture 1: target is inf",[](SchroHipQuantChoosePicture & p) { p.target = INFINITY; }},
    {"picture 1: engine 9 is unknown",[](SchroHipQuantChoosePicture & p) { p.engine = 9; }},
    {"picture 1: counts[1] is NULL",[](SchroHipQuantChoosePicture & p) { p.counts[1] = nullptr; }},
    {"picture 1: result is NULL or not 8-byte aligned",[](SchroHipQuantChoosePicture & p) { p.result = (SchroHipQuantChoice *) ((char *) p.result + 4); }},
    {"picture 1: is_noarith 0 needs",[](SchroHipQuantChoosePicture & p) { p.is_noarith = 0; }},
  };
  int nbad = 0;
  for (const Bad & b:bads) {
    SchroHipQuantChoosePicture two[2] = { one, one };
    b.make (two[1]);
    EXPECT (refused (schro_hip_quant_choose_check (two, 2, 0), b.fragment), "not refused: %s", b.fragment);
    nbad++;
  }

  // ---- batches: the queue's scratch small, large, small, on two queues; unlike depths, forms and engines
  int batches = 0;
  for (int queue = 0; queue < 2; queue++) {
    EXPECT (schro_hip_context_select_queue (ctx, queue) == 0, "select queue %d", queue);
    for (int n:{ 1, 9, 1 }) {
      std::vector < SchroHipQuantChoosePicture > pics;
      for (int k = 0; k < n; k++)
        pics.push_back (choose_picture (ctx, (k * 5 + queue) % 7, k % 3, (k >> 1) & 1, owned));
      pics[0].est_entropy = (double *) take (ctx, sizeof (double) * 3 * 19 * 60);
      pics[0].est_error = (double *) take (ctx, sizeof (double) * 3 * 19 * 60);
      owned.push_back (pics[0].est_entropy);
      owned.push_back (pics[0].est_error);
      EXPECT (schro_hip_quant_choose_batch (ctx, pics.data (), n) == 0, "a batch of %d on queue %d", n, queue);
      batches++;
    }
  }
  EXPECT (schro_hip_context_select_queue (ctx, 0) == 0, "select queue 0");

  // ---- the consumers: a 32 x 16 4:4:4 picture of depth 2, records that carry their sub-band
  const int depth = 2, w = 32, h = 16, bpp = 2, stride = w * bpp;
  const int hc[7] = { 1, 2, 2 }, vc[7] = { 1, 1, 2 };
  const int nrec = schro_hip_codeblock_layout (w, h, depth, hc, vc, stride, bpp, nullptr, 0);
  EXPECT (nrec == 1 + 3 * 2 + 3 * 4, "%d records", nrec);
  std::vector < SchroHipCodeblock > recs ((size_t) nrec);
  schro_hip_codeblock_layout (w, h, depth, hc, vc, stride, bpp, recs.data (), nrec);
  {
    int n = 0;
    for (int i = 0; i < 1 + 3 * depth; i++) {
      const int level = i == 0 ? 0 : (i - 1) / 3 + 1;
      for (int k = 0; k < hc[level] * vc[level]; k++)
        recs[n++].quant_index = (unsigned char) i;
    }
  }
  SchroHipQuantChoice *choice = (SchroHipQuantChoice *) take (ctx, sizeof (SchroHipQuantChoice));
  uint32_t *clamped = (uint32_t *) take (ctx, 2 * sizeof (uint32_t));
  owned.push_back (choice);
  owned.push_back (clamped);
  SchroHipQuantPlane planes[3];
  SchroHipNoarithPicture pic;
  memset (planes, 0, sizeof (planes));
  memset (&pic, 0, sizeof (pic));
  const int32_t *rows[3];
  for (int c = 0; c < 3; c++) {
    planes[c].coeffs = take (ctx, (size_t) stride * h);
    planes[c].quant = take (ctx, (size_t) stride * h);
    planes[c].bytes = (size_t) stride * h;
    planes[c].codeblocks = recs.data ();
    planes[c].ncodeblocks = nrec;
    planes[c].is_intra = 1;
    planes[c].dc_predict_first = 1;
    planes[c].dc_width = w >> depth;
    planes[c].dc_height = h >> depth;
    planes[c].summary = (SchroHipCodeblockSummary *) take (ctx, sizeof (SchroHipCodeblockSummary) * nrec);
    owned.push_back (planes[c].coeffs);
    owned.push_back (planes[c].quant);
    owned.push_back (planes[c].summary);
    rows[c] = choice->quant_index[c];
    pic.quant[c] = planes[c].quant;
    pic.bytes[c] = planes[c].bytes;
    pic.stride[c] = stride;
    pic.iwt_width[c] = w;
    pic.iwt_height[c] = h;
    pic.codeblocks[c] = recs.data ();
    pic.ncodeblocks[c] = nrec;
  }
  pic.transform_depth = depth;
  memcpy (pic.horiz_codeblocks, hc, sizeof (hc));
  memcpy (pic.vert_codeblocks, vc, sizeof (vc));
  pic.codeblock_mode_index = 1;
  const int64_t bound = schro_hip_noarith_encode_bound (&pic, bpp);
  EXPECT (bound > 0, "bound %lld", (long long) bound);
  pic.out = (uint8_t *) take (ctx, (size_t) bound);
  pic.capacity = (size_t) bound;
  pic.result = (SchroHipNoarithResult *) take (ctx, sizeof (SchroHipNoarithResult));
  owned.push_back (pic.out);
  owned.push_back (pic.result);
  const int32_t *whole = &choice->quant_index[0][0];

  EXPECT (schro_hip_quantise_chosen_batch (ctx, planes, rows, 3, bpp, clamped) == 0, "quantise_chosen_batch");
  EXPECT (schro_hip_noarith_encode_chosen_check (&pic, &whole, 1, bpp, clamped + 1) == 0, "noarith_encode_chosen_check");
  EXPECT (schro_hip_noarith_encode_chosen_batch (ctx, &pic, &whole, 1, bpp, clamped + 1) == 0, "noarith_encode_chosen_batch");
  // (the entry points that take host indices still take these records: a sub-band number is a legal index; the VLC
  // encoder's one-index-per-sub-band rule holds too)
  EXPECT (schro_hip_quantise_batch (ctx, planes, 3, bpp) == 0, "quantise_batch");
  EXPECT (schro_hip_noarith_encode_batch (ctx, &pic, 1, bpp) == 0, "noarith_encode_batch");
  // refusals of the chosen form
  EXPECT (refused (schro_hip_quantise_chosen_batch (ctx, planes, nullptr, 3, bpp, clamped), "chosen is NULL"), "chosen NULL");
  EXPECT (refused (schro_hip_quantise_chosen_batch (ctx, planes, rows, 3, bpp, nullptr), "clamped is NULL"), "clamped NULL");
  {
    const int32_t *odd[3] = { rows[0], (const int32_t *) ((const char *) rows[1] + 2), rows[2] };
    EXPECT (refused (schro_hip_quantise_chosen_batch (ctx, planes, odd, 3, bpp, clamped), "plane 1: chosen is NULL or not 4-byte aligned"),
        "odd chosen");
    std::vector < SchroHipCodeblock > bad (recs);
    bad[4].quant_index = 19;
    SchroHipQuantPlane bp = planes[2];
    bp.codeblocks = bad.data ();
    EXPECT (refused (schro_hip_quantise_chosen_batch (ctx, &bp, rows + 2, 1, bpp, clamped), "codeblock 4: quant_index 19 is no sub-band"),
        "a sub-band of 19");
    bad[4].quant_index = 1;
    SchroHipNoarithPicture bpic = pic;
    bpic.codeblocks[1] = bad.data ();
    EXPECT (refused (schro_hip_noarith_encode_chosen_check (&bpic, &whole, 1, bpp, clamped), "component 1, sub-band 2, record 4: quant_index 1 is not the sub-band"),
        "a record of another sub-band");
    const int32_t *none = nullptr;
    EXPECT (refused (schro_hip_noarith_encode_chosen_check (&pic, &none, 1, bpp, clamped), "picture 0: chosen is NULL"), "a NULL row");
    EXPECT (refused (schro_hip_noarith_encode_chosen_batch (ctx, &pic, &whole, 1, bpp, nullptr), "clamped is NULL"), "clamped NULL (VLC)");
  }

  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  for (void *m:owned)
    schro_hip_domain_free (ctx, m);
  schro_hip_context_free (ctx);
  if (failures) {
    fprintf (stderr, "quant_choose_walk: %d failures\n", failures);
    return 1;
  }
  printf ("quant_choose_walk: %d refusals, %d batches, the chosen consumers, ok\n", nbad, batches);
  return 0;
}
