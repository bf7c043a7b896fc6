// noarith_walk.cpp -- the host code of the noarith transform-data encoder (plane_noarith_enc.cpp and the frame layer's
// schro_hip_encode_transform_data_noarith) walked under AddressSanitizer + UndefinedBehaviorSanitizer: a plain C++ program
// with its own main, linked with the objects of the library's device-free sanitizer build (make -C schroedinger_amd/csrc
// dry_asan).  Launches are dropped there, so what runs is every refusal, the record comparison, the table and scratch
// arithmetic.  The pictures and the refusals are the case module's: tests/test_noarith_host_sanitized.py writes
// tests/noarith_enc_cases.py's geometries and descriptions into the table this program reads (argv[1]):
//   G name bpp depth mode w0 h0 w1 h1 w2 h2 hc[7] vc[7]                     a geometry: laid out, checked, run
//   D name refused bpp depth mode w0 h0 w1 h1 w2 h2 hc[7] vc[7] stride[3] bytes[3] quant[3] out capacity result n[3]
//   r dst_offset dst_stride width height quant_index                         ... its n[0] + n[1] + n[2] records
//   M fragment of the message (the rest of the line)                         ... and what the refusal must say
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "noarith_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

struct Geometry {
  std::string name;
  int bpp;
  SchroHipNoarithPicture p;
  std::vector < SchroHipCodeblock > recs[3];
  std::vector < void *>owned;
};

static void
read_shape (FILE * f, SchroHipNoarithPicture & p, int *bpp)
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
    fprintf (stderr, "noarith_walk: bad table\n");
    exit (2);
  }
}

static void *
take (SchroHipContext * ctx, Geometry & g, size_t bytes)
{
  void *m = schro_hip_domain_alloc (ctx, bytes + 256);
  if (!m) {
    fprintf (stderr, "noarith_walk: no memory: %s\n", schro_hip_last_error ());
    exit (2);
  }
  g.owned.push_back (m);
  return m;
}

static void
lay_out (SchroHipContext * ctx, Geometry & g)
{
  SchroHipNoarithPicture & p = g.p;
  for (int k = 0; k < 3; k++) {
    p.stride[k] = (p.iwt_width[k] * g.bpp + 63) / 64 * 64;
    p.bytes[k] = (size_t) p.stride[k] * p.iwt_height[k];
    p.quant[k] = take (ctx, g, p.bytes[k]);
    const int n = schro_hip_codeblock_layout (p.iwt_width[k], p.iwt_height[k], p.transform_depth, p.horiz_codeblocks, p.vert_codeblocks,
        p.stride[k], g.bpp, nullptr, 0);
    EXPECT (n > 0, "%s: no layout", g.name.c_str ());
    g.recs[k].resize (n > 0 ? n : 1);
    schro_hip_codeblock_layout (p.iwt_width[k], p.iwt_height[k], p.transform_depth, p.horiz_codeblocks, p.vert_codeblocks, p.stride[k],
        g.bpp, g.recs[k].data (), n);
    // one quant index per sub-band: a record's sub-band is found from its pitch and offset no easier than by counting
    int at = 0;
    for (int i = 0; i < 1 + 3 * p.transform_depth; i++) {
      const int level = i == 0 ? 0 : (i - 1) / 3 + 1;
      const int count = p.horiz_codeblocks[level] * p.vert_codeblocks[level];
      for (int c = 0; c < count && at < n; c++, at++)
        g.recs[k][at].quant_index = (unsigned char) ((5 * i + k) % 61);
    }
    p.codeblocks[k] = g.recs[k].data ();
    p.ncodeblocks[k] = n;
  }
  const int64_t bound = schro_hip_noarith_encode_bound (&p, g.bpp);
  EXPECT (bound > 0, "%s: bound %lld", g.name.c_str (), (long long) bound);
  p.capacity = bound > 0 ? (size_t) bound : 1;
  p.out = (uint8_t *) take (ctx, g, p.capacity);
  p.result = (SchroHipNoarithResult *) take (ctx, g, sizeof (SchroHipNoarithResult));
}

int
main (int argc, char **argv)
{
  FILE *f = argc > 1 ? fopen (argv[1], "r") : nullptr;
  if (!f) {
    fprintf (stderr, "noarith_walk: needs the table\n");
    return 2;
  }
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "noarith_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
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
      lay_out (ctx, *g);
      EXPECT (schro_hip_noarith_encode_check (&g->p, 1, g->bpp) == 0, "%s is refused", name);
      EXPECT (schro_hip_noarith_encode_batch (ctx, &g->p, 1, g->bpp) == 0, "%s does not run", name);
      // one byte short of the bound and no room at all are capacities like any other
      SchroHipNoarithPicture tight = g->p;
      tight.capacity = 0;
      EXPECT (schro_hip_noarith_encode_batch (ctx, &tight, 1, g->bpp) == 0, "%s does not run without room", name);
      geometries.push_back (g);
    } else if (kind[0] == 'D') {
      int refused, bpp, n[3];
      SchroHipNoarithPicture p;
      if (fscanf (f, "%d", &refused) != 1)
        return 2;
      read_shape (f, p, &bpp);
      unsigned long long quant[3], bytes[3], out, capacity, result;
      int ok = 0;
      for (int k = 0; k < 3; k++)
        ok += fscanf (f, "%d", &p.stride[k]);
      for (int k = 0; k < 3; k++)
        ok += fscanf (f, "%llu", &bytes[k]);
      for (int k = 0; k < 3; k++)
        ok += fscanf (f, "%llu", &quant[k]);
      ok += fscanf (f, "%llu %llu %llu %d %d %d", &out, &capacity, &result, &n[0], &n[1], &n[2]);
      if (ok != 15)
        return 2;
      std::vector < SchroHipCodeblock > recs[3];
      for (int k = 0; k < 3; k++) {
        recs[k].resize (n[k] + 1);
        for (int c = 0; c < n[k]; c++) {
          SchroHipCodeblock & cb = recs[k][c];
          int qi;
          memset (&cb, 0, sizeof (cb));
          if (fscanf (f, " r %d %d %d %d %d", &cb.dst_offset, &cb.dst_stride, &cb.width, &cb.height, &qi) != 5)
            return 2;
          cb.src_offset = -1;
          cb.quant_index = (unsigned char) qi;
        }
        // (addresses only: the check dereferences nothing but the records)
        p.quant[k] = (const void *) (uintptr_t) quant[k];
        p.bytes[k] = (size_t) bytes[k];
        p.codeblocks[k] = recs[k].data ();
        p.ncodeblocks[k] = n[k];
      }
      p.out = (uint8_t *) (uintptr_t) out;
      p.capacity = (size_t) capacity;
      p.result = (SchroHipNoarithResult *) (uintptr_t) result;
      char message[256] = "";
      if (fscanf (f, " M %255[^\n]", message) != 1)
        message[0] = 0;
      const int r = schro_hip_noarith_encode_check (&p, 1, bpp);
      if (refused) {
        EXPECT (r == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), message), "%s: passes, or does not say \"%s\"", name, message);
        EXPECT (schro_hip_noarith_encode_batch (ctx, &p, 1, bpp) == SCHRO_HIP_EINVAL, "%s: the batch runs it", name);
      } else {
        EXPECT (r == 0, "%s is refused", name);
      }
      descriptions++;
    } else {
      fprintf (stderr, "noarith_walk: bad table line %s\n", kind);
      return 2;
    }
  }
  fclose (f);
  // every geometry of a sample size in one call
  for (int bpp = 2; bpp <= 4; bpp += 2) {
    std::vector < SchroHipNoarithPicture > batch;
    for (Geometry * g:geometries)
      if (g->bpp == bpp)
        batch.push_back (g->p);
    if (!batch.empty ())
      EXPECT (schro_hip_noarith_encode_batch (ctx, batch.data (), (int) batch.size (), bpp) == 0, "batch of %zu", batch.size ());
  }
  if (!geometries.empty ()) {
    Geometry & g = *geometries[0];
    EXPECT (schro_hip_noarith_encode_batch (nullptr, &g.p, 1, g.bpp) == SCHRO_HIP_EINVAL, "no context passes");
    EXPECT (schro_hip_noarith_encode_check (nullptr, 1, 2) == SCHRO_HIP_EINVAL, "no pictures pass");
    EXPECT (schro_hip_noarith_encode_check (&g.p, 0, g.bpp) == SCHRO_HIP_EINVAL, "an empty call passes");
    EXPECT (schro_hip_noarith_encode_bound (nullptr, 2) == SCHRO_HIP_EINVAL, "a bound of nothing");
    EXPECT (schro_hip_encode_transform_data_noarith (nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == SCHRO_HIP_EINVAL,
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
  printf ("noarith_walk: %zu geometries, %d descriptions, %s\n", count, descriptions, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
