// motion_arith_dec_walk.cpp -- the host code of the arithmetic motion-data decoder (plane_motion_arith_dec.cpp and the frame
// layer's schro_hip_decode_motion_data_arith) walked under AddressSanitizer + UndefinedBehaviorSanitizer: a plain C++
// program with its own main, linked with the objects of the library's device-free sanitizer build (make -C
// schroedinger_amd/csrc dry_asan), in the form of motion_dec_walk.cpp.  Launches are dropped there, so what runs is every
// refusal, the overlap test, the table and scratch arithmetic and the frame layer's copies and its refusal of a noarith
// picture.  The geometries, the refusals and the scratch counts are the case module's:
// tests/test_motion_arith_dec_host_sanitized.py writes them into the table this program reads (argv[1]):
//   G name x_num_blocks y_num_blocks num_refs have_global_motion data_bytes words     a geometry: laid out, checked, run;
//                                                                                     `words`: the scratch it takes
//   D name refused pictures words                                     a description of `pictures` pictures ...
//   p data data_bytes bytes_on_device x_num_blocks y_num_blocks num_refs have_global_motion motion result   ... each
//                                                                                     (addresses only)
//   M fragment of the message (the rest of the line)                  ... and what the refusal must say
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "motion_arith_dec_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

struct Geometry {
  std::string name;
  SchroHipMotionArithDecodePicture p;
  std::vector < void *>owned;
};

static void *
take (SchroHipContext * ctx, Geometry & g, size_t bytes)
{
  void *m = schro_hip_domain_alloc (ctx, bytes + 256);
  if (!m) {
    fprintf (stderr, "motion_arith_dec_walk: no memory: %s\n", schro_hip_last_error ());
    exit (2);
  }
  g.owned.push_back (m);
  return m;
}

int
main (int argc, char **argv)
{
  FILE *f = argc > 1 ? fopen (argv[1], "r") : nullptr;
  if (!f) {
    fprintf (stderr, "motion_arith_dec_walk: needs the table\n");
    return 2;
  }
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "motion_arith_dec_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
    return 2;
  }
  std::vector < Geometry * >geometries;
  int descriptions = 0;
  long long batch_words = 0;
  char kind[8], name[128];
  while (fscanf (f, "%7s %127s", kind, name) == 2) {
    if (kind[0] == 'G') {
      Geometry *g = new Geometry ();
      g->name = name;
      SchroHipMotionArithDecodePicture & p = g->p;
      memset (&p, 0, sizeof (p));
      unsigned long long data_bytes;
      long long words;
      if (fscanf (f, "%d %d %d %d %llu %lld", &p.x_num_blocks, &p.y_num_blocks, &p.num_refs, &p.have_global_motion, &data_bytes, &words) != 6)
        return 2;
      const size_t field_bytes = (size_t) p.x_num_blocks * p.y_num_blocks * 20;
      p.data_bytes = (size_t) data_bytes;
      p.data = (const uint8_t *) take (ctx, *g, p.data_bytes + 1) + 1;   // (an odd address)
      p.motion = take (ctx, *g, field_bytes);
      p.result = (SchroHipMotionArithDecodeResult *) take (ctx, *g, sizeof (SchroHipMotionArithDecodeResult));
      EXPECT (schro_hip_motion_arith_decode_check (&p, 1) == 0, "%s is refused", name);
      EXPECT (schro_hip_motion_arith_decode_scratch_words (&p, 1) == words, "%s: %lld words of scratch, the hand count is %lld", name,
          (long long) schro_hip_motion_arith_decode_scratch_words (&p, 1), words);
      batch_words += words;
      EXPECT (schro_hip_motion_arith_decode_batch (ctx, &p, 1) == 0, "%s does not run", name);
      // a length word and no bytes at all
      SchroHipMotionArithDecodePicture other = p;
      other.bytes_on_device = (const uint32_t *) take (ctx, *g, 4);
      other.data_bytes = 0;
      EXPECT (schro_hip_motion_arith_decode_batch (ctx, &other, 1) == 0, "%s does not run without bytes", name);
      // the frame layer on host bytes and a host field of the same geometry
      std::vector < uint8_t > field (field_bytes, 0), bytes (p.data_bytes + 1, 0x80);
      SchroHipMotion motion;
      SchroHipParams params;
      memset (&motion, 0, sizeof (motion));
      memset (&params, 0, sizeof (params));
      motion.motion_vectors = field.data ();
      params.x_num_blocks = p.x_num_blocks;
      params.y_num_blocks = p.y_num_blocks;
      params.num_refs = p.num_refs;
      params.have_global_motion = p.have_global_motion;
      SchroHipMotionArithDecodeResult result;
      EXPECT (schro_hip_decode_motion_data_arith (ctx, bytes.data (), p.data_bytes, &params, &motion, &result) == 0,
          "%s: the frame layer does not run", name);
      EXPECT (schro_hip_decode_motion_data_arith (ctx, nullptr, 0, &params, &motion, nullptr) == 0,
          "%s: the frame layer does not run without bytes", name);
      params.is_noarith = 1;
      EXPECT (schro_hip_decode_motion_data_arith (ctx, bytes.data (), p.data_bytes, &params, &motion, &result) == SCHRO_HIP_EINVAL,
          "%s: the frame layer takes a noarith picture", name);
      geometries.push_back (g);
    } else if (kind[0] == 'D') {
      int refused, n;
      long long words;
      if (fscanf (f, "%d %d %lld", &refused, &n, &words) != 3 || n < 1 || n > 8)
        return 2;
      std::vector < SchroHipMotionArithDecodePicture > pics (n);
      for (int k = 0; k < n; k++) {
        SchroHipMotionArithDecodePicture & p = pics[k];
        memset (&p, 0, sizeof (p));
        unsigned long long data, data_bytes, word, motion, result;
        // (addresses only: the check dereferences nothing)
        if (fscanf (f, " p %llu %llu %llu %d %d %d %d %llu %llu", &data, &data_bytes, &word, &p.x_num_blocks, &p.y_num_blocks, &p.num_refs,
                &p.have_global_motion, &motion, &result) != 9)
          return 2;
        p.data = (const uint8_t *) (uintptr_t) data;
        p.data_bytes = (size_t) data_bytes;
        p.bytes_on_device = (const uint32_t *) (uintptr_t) word;
        p.motion = (void *) (uintptr_t) motion;
        p.result = (SchroHipMotionArithDecodeResult *) (uintptr_t) result;
      }
      char message[256] = "";
      if (fscanf (f, " M %255[^\n]", message) != 1)
        message[0] = 0;
      const int r = schro_hip_motion_arith_decode_check (pics.data (), n);
      if (refused) {
        EXPECT (r == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), message), "%s: passes, or does not say \"%s\"", name, message);
        EXPECT (schro_hip_motion_arith_decode_batch (ctx, pics.data (), n) == SCHRO_HIP_EINVAL, "%s: the batch runs it", name);
        EXPECT (schro_hip_motion_arith_decode_scratch_words (pics.data (), n) == SCHRO_HIP_EINVAL, "%s: has a scratch size", name);
      } else {
        EXPECT (r == 0, "%s is refused", name);
        EXPECT (schro_hip_motion_arith_decode_scratch_words (pics.data (), n) == words, "%s: %lld words of scratch, the hand count is %lld", name,
            (long long) schro_hip_motion_arith_decode_scratch_words (pics.data (), n), words);
      }
      descriptions++;
    } else {
      fprintf (stderr, "motion_arith_dec_walk: bad table line %s\n", kind);
      return 2;
    }
  }
  fclose (f);
  // every geometry in one call
  std::vector < SchroHipMotionArithDecodePicture > batch;
  for (Geometry * g:geometries)
    batch.push_back (g->p);
  if (!batch.empty ()) {
    EXPECT (schro_hip_motion_arith_decode_scratch_words (batch.data (), (int) batch.size ()) == batch_words, "the batch's scratch is not the sum");
    EXPECT (schro_hip_motion_arith_decode_batch (ctx, batch.data (), (int) batch.size ()) == 0, "batch of %zu", batch.size ());
  }
  if (!geometries.empty ()) {
    Geometry & g = *geometries[0];
    EXPECT (schro_hip_motion_arith_decode_batch (nullptr, &g.p, 1) == SCHRO_HIP_EINVAL, "no context passes");
    EXPECT (schro_hip_motion_arith_decode_check (nullptr, 1) == SCHRO_HIP_EINVAL, "no pictures pass");
    EXPECT (schro_hip_motion_arith_decode_check (&g.p, 0) == SCHRO_HIP_EINVAL, "an empty call passes");
    EXPECT (schro_hip_decode_motion_data_arith (nullptr, nullptr, 0, nullptr, nullptr, nullptr) == SCHRO_HIP_EINVAL,
        "the frame call without a context passes");
  }
  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  const size_t count = geometries.size ();
  for (Geometry * g:geometries) {
    for (void *m:g->owned)
      schro_hip_domain_free (ctx, m);
    delete g;
  }
  schro_hip_context_free (ctx);
  printf ("motion_arith_dec_walk: %zu geometries, %d descriptions, %s\n", count, descriptions, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
