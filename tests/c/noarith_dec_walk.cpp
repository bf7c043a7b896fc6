// noarith_dec_walk.cpp -- the host code of the noarith transform-data decoder (plane_noarith_dec.cpp and the frame layer's
// schro_hipframe_decode_transform_data_noarith) walked under AddressSanitizer + UndefinedBehaviorSanitizer: a plain C++
// program with its own main, linked with the objects of the library's device-free sanitizer build (make -C
// schroedinger_amd/csrc dry_asan).  Launches are dropped there, so what runs is every refusal and the table and scratch
// arithmetic.  The pictures and the refusals are the case module's: tests/test_noarith_dec_host_sanitized.py writes
// tests/noarith_dec_cases.py's geometries and descriptions into the table this program reads (argv[1]):
//   G name bpp depth mode w0 h0 w1 h1 w2 h2 hc[7] vc[7] data_bytes scratch_words       a geometry: laid out, checked, run
//   D name refused bpp depth mode w0 h0 w1 h1 w2 h2 hc[7] vc[7] stride[3] bytes[3] coeffs[3] quant[3] data data_bytes
//     bytes_on_device result
//   M fragment of the message (the rest of the line)                                   ... what the refusal must say
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "noarith_dec_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

struct Geometry {
  std::string name;
  int bpp;
  SchroHipNoarithDecodePicture p;
  std::vector < void *>owned;
};

static void
read_shape (FILE * f, SchroHipNoarithDecodePicture & p, int *bpp)
{
  memset (&p, 0, sizeof (p));
  int ok = fscanf (f, "%d %d %d", bpp, &p.transform_depth, &p.codeblock_mode_index);
  for (int k = 0; k < 3; k++)
    ok += fscanf (f, "%d %d", &p.iwt_width[k], &p.iwt_height[k]);
  for (int l = 0; l < 7; l++)
    ok += fscanf (f, "%d", &p.horiz_codeblocks[l]);
  for (int l = 0; l < 7; l++)
    ok += fscanf (f, "%d", &p.vert_codeblocks[l]);
  if (ok != 23) {
    fprintf (stderr, "noarith_dec_walk: bad table\n");
    exit (2);
  }
}

static void *
take (SchroHipContext * ctx, Geometry & g, size_t bytes)
{
  void *m = schro_hip_domain_alloc (ctx, bytes + 256);
  if (!m) {
    fprintf (stderr, "noarith_dec_walk: no memory: %s\n", schro_hip_last_error ());
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
    fprintf (stderr, "noarith_dec_walk: needs the table\n");
    return 2;
  }
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "noarith_dec_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
    return 2;
  }
  std::vector < Geometry * >geometries;
  int descriptions = 0;
  char kind[8], name[128];
  while (fscanf (f, "%7s %127s", kind, name) == 2) {
    if (kind[0] == 'G') {
      Geometry *g = new Geometry ();
      g->name = name;
      read_shape (f, g->p, &g->bpp);
      unsigned long long data_bytes, words;
      if (fscanf (f, "%llu %llu", &data_bytes, &words) != 2)
        return 2;
      SchroHipNoarithDecodePicture & p = g->p;
      for (int k = 0; k < 3; k++) {
        p.stride[k] = (p.iwt_width[k] * g->bpp + 63) / 64 * 64;
        p.bytes[k] = (size_t) p.stride[k] * p.iwt_height[k];
        p.coeffs[k] = take (ctx, *g, p.bytes[k]);
        p.quant[k] = take (ctx, *g, p.bytes[k]);
      }
      p.data = (const uint8_t *) take (ctx, *g, data_bytes);
      p.data_bytes = (size_t) data_bytes;
      p.result = (SchroHipNoarithDecodeResult *) take (ctx, *g, sizeof (SchroHipNoarithDecodeResult));
      EXPECT (schro_hip_noarith_decode_check (&p, 1, g->bpp) == 0, "%s is refused", name);
      // the scratch formula: 5 words per chunk slot, 3 per codeblock, 8 per sub-band, 2 per picture
      const long long got = schro_hip_noarith_decode_scratch_words (&p, 1, g->bpp);
      EXPECT (got == (long long) words, "%s: %lld words of scratch, the formula says %llu", name, got, words);
      EXPECT (schro_hip_noarith_decode_batch (ctx, &p, 1, g->bpp) == 0, "%s does not run", name);
      // the length word on the device, no quant planes, no input at all
      SchroHipNoarithDecodePicture other = p;
      other.bytes_on_device = (const uint32_t *) take (ctx, *g, 4);
      other.quant[0] = other.quant[1] = other.quant[2] = nullptr;
      EXPECT (schro_hip_noarith_decode_batch (ctx, &other, 1, g->bpp) == 0, "%s does not run without quant planes", name);
      other.data_bytes = 0;
      EXPECT (schro_hip_noarith_decode_batch (ctx, &other, 1, g->bpp) == 0, "%s does not run without input", name);
      geometries.push_back (g);
    } else if (kind[0] == 'D') {
      int refused, bpp;
      SchroHipNoarithDecodePicture p;
      if (fscanf (f, "%d", &refused) != 1)
        return 2;
      read_shape (f, p, &bpp);
      unsigned long long coeffs[3], quant[3], bytes[3], data, data_bytes, on_device, result;
      int ok = 0;
      for (int k = 0; k < 3; k++)
        ok += fscanf (f, "%d", &p.stride[k]);
      for (int k = 0; k < 3; k++)
        ok += fscanf (f, "%llu", &bytes[k]);
      for (int k = 0; k < 3; k++)
        ok += fscanf (f, "%llu", &coeffs[k]);
      for (int k = 0; k < 3; k++)
        ok += fscanf (f, "%llu", &quant[k]);
      ok += fscanf (f, "%llu %llu %llu %llu", &data, &data_bytes, &on_device, &result);
      if (ok != 16)
        return 2;
      // (addresses only: the check dereferences nothing)
      for (int k = 0; k < 3; k++) {
        p.coeffs[k] = (void *) (uintptr_t) coeffs[k];
        p.quant[k] = (void *) (uintptr_t) quant[k];
        p.bytes[k] = (size_t) bytes[k];
      }
      p.data = (const uint8_t *) (uintptr_t) data;
      p.data_bytes = (size_t) data_bytes;
      p.bytes_on_device = (const uint32_t *) (uintptr_t) on_device;
      p.result = (SchroHipNoarithDecodeResult *) (uintptr_t) result;
      char message[256] = "";
      if (fscanf (f, " M %255[^\n]", message) != 1)
        message[0] = 0;
      const int r = schro_hip_noarith_decode_check (&p, 1, bpp);
      if (refused) {
        EXPECT (r == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), message), "%s: passes, or does not say \"%s\"", name, message);
        EXPECT (schro_hip_noarith_decode_batch (ctx, &p, 1, bpp) == SCHRO_HIP_EINVAL, "%s: the batch runs it", name);
        EXPECT (schro_hip_noarith_decode_scratch_words (&p, 1, bpp) == SCHRO_HIP_EINVAL, "%s: has a scratch size", name);
      } else {
        EXPECT (r == 0, "%s is refused", name);
      }
      descriptions++;
    } else {
      fprintf (stderr, "noarith_dec_walk: bad table line %s\n", kind);
      return 2;
    }
  }
  fclose (f);
  // every geometry of a sample size in one call
  for (int bpp = 2; bpp <= 4; bpp += 2) {
    std::vector < SchroHipNoarithDecodePicture > batch;
    for (Geometry * g:geometries)
      if (g->bpp == bpp)
        batch.push_back (g->p);
    while (batch.size () > 64)
      batch.pop_back ();
    if (!batch.empty ())
      EXPECT (schro_hip_noarith_decode_batch (ctx, batch.data (), (int) batch.size (), bpp) == 0, "batch of %zu", batch.size ());
  }
  if (!geometries.empty ()) {
    Geometry & g = *geometries[0];
    int compat = 0;
    SchroHipNoarithDecodeResult result;
    EXPECT (schro_hip_noarith_decode_batch (nullptr, &g.p, 1, g.bpp) == SCHRO_HIP_EINVAL, "no context passes");
    EXPECT (schro_hip_noarith_decode_check (nullptr, 1, 2) == SCHRO_HIP_EINVAL, "no pictures pass");
    EXPECT (schro_hip_noarith_decode_check (&g.p, 0, g.bpp) == SCHRO_HIP_EINVAL, "an empty call passes");
    EXPECT (schro_hipframe_decode_transform_data_noarith (nullptr, nullptr, 0, nullptr, &compat, &result) == SCHRO_HIP_EINVAL,
        "the frame call without a frame passes");
  }
  EXPECT (schro_hip_synchronize (ctx) == 0, "synchronize");
  const size_t count = geometries.size ();
  for (Geometry * g:geometries) {
    for (void *m:g->owned)
      schro_hip_domain_free (ctx, m);
    delete g;
  }
  schro_hip_context_free (ctx);
  printf ("noarith_dec_walk: %zu geometries, %d descriptions, %s\n", count, descriptions, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
