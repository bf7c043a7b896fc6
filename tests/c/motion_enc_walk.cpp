// motion_enc_walk.cpp -- the host code of the motion-data encoder (plane_motion_enc.cpp and the frame layer's
// schro_hip_encode_motion_data_noarith) walked under AddressSanitizer + UndefinedBehaviorSanitizer: a plain C++ program
// with its own main, linked with the objects of the library's device-free sanitizer build (make -C schroedinger_amd/csrc
// dry_asan).  Launches are dropped there, so what runs is every refusal, the overlap test, the bound, the table and
// scratch arithmetic and the frame layer's copies.  The geometries and the refusals are the case module's:
// tests/test_motion_enc_host_sanitized.py writes them into the table this program reads (argv[1]):
//   G name x_num_blocks y_num_blocks num_refs have_global_motion            a geometry: laid out, checked, run
//   D name refused pictures                                                 a description of `pictures` pictures ...
//   p motion x_num_blocks y_num_blocks num_refs have_global_motion out capacity result   ... each (addresses only)
//   M fragment of the message (the rest of the line)                        ... and what the refusal must say
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "schro_hip.h"

static int failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf (stderr, "motion_enc_walk: " __VA_ARGS__); fprintf (stderr, " [%s]\n", schro_hip_last_error ()); } } while (0)

struct Geometry {
  std::string name;
  SchroHipMotionEncodePicture p;
  std::vector < void *>owned;
};

static void *
take (SchroHipContext * ctx, Geometry & g, size_t bytes)
{
  void *m = schro_hip_domain_alloc (ctx, bytes + 256);
  if (!m) {
    fprintf (stderr, "motion_enc_walk: no memory: %s\n", schro_hip_last_error ());
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
    fprintf (stderr, "motion_enc_walk: needs the table\n");
    return 2;
  }
  SchroHipContext *ctx = schro_hip_context_new (0);
  if (!ctx) {
    fprintf (stderr, "motion_enc_walk: schro_hip_context_new: %s\n", schro_hip_last_error ());
    return 2;
  }
  std::vector < Geometry * >geometries;
  int descriptions = 0;
  char kind[8], name[128];
  while (fscanf (f, "%7s %127s", kind, name) == 2) {
    if (kind[0] == 'G') {
      Geometry *g = new Geometry ();
      g->name = name;
      SchroHipMotionEncodePicture & p = g->p;
      memset (&p, 0, sizeof (p));
      if (fscanf (f, "%d %d %d %d", &p.x_num_blocks, &p.y_num_blocks, &p.num_refs, &p.have_global_motion) != 4)
        return 2;
      const int64_t bound = schro_hip_motion_encode_bound (p.x_num_blocks, p.y_num_blocks, p.num_refs, p.have_global_motion);
      EXPECT (bound > 0, "%s: bound %lld", name, (long long) bound);
      const size_t field_bytes = (size_t) p.x_num_blocks * p.y_num_blocks * 20;
      p.motion = take (ctx, *g, field_bytes);
      p.capacity = bound > 0 ? (size_t) bound : 1;
      p.out = (uint8_t *) take (ctx, *g, p.capacity);
      p.result = (SchroHipMotionEncodeResult *) take (ctx, *g, sizeof (SchroHipMotionEncodeResult));
      EXPECT (schro_hip_motion_encode_check (&p, 1) == 0, "%s is refused", name);
      EXPECT (schro_hip_motion_encode_batch (ctx, &p, 1) == 0, "%s does not run", name);
      // no room at all and an odd address are outputs like any other
      SchroHipMotionEncodePicture tight = p;
      tight.capacity = 0;
      tight.out += 1;
      EXPECT (schro_hip_motion_encode_batch (ctx, &tight, 1) == 0, "%s does not run without room", name);
      // the frame layer on a host field of the same geometry
      std::vector < uint8_t > field (field_bytes, 0), bytes ((size_t) p.capacity);
      SchroHipMotion motion;
      SchroHipParams params;
      memset (&motion, 0, sizeof (motion));
      memset (&params, 0, sizeof (params));
      motion.motion_vectors = field.data ();
      params.x_num_blocks = p.x_num_blocks;
      params.y_num_blocks = p.y_num_blocks;
      params.num_refs = p.num_refs;
      params.have_global_motion = p.have_global_motion;
      size_t taken = 0;
      int sections[SCHRO_HIP_MOTION_SECTIONS];
      SchroHipMotionEncodeResult result;
      EXPECT (schro_hip_encode_motion_data_noarith (ctx, &motion, &params, bytes.data (), bytes.size (), &taken, sections, &result) == 0,
          "%s: the frame layer does not run", name);
      EXPECT (schro_hip_encode_motion_data_noarith (ctx, &motion, &params, nullptr, 0, &taken, nullptr, nullptr) == 0,
          "%s: the frame layer does not run without room", name);
      geometries.push_back (g);
    } else if (kind[0] == 'D') {
      int refused, n;
      if (fscanf (f, "%d %d", &refused, &n) != 2 || n < 1 || n > 8)
        return 2;
      std::vector < SchroHipMotionEncodePicture > pics (n);
      for (int k = 0; k < n; k++) {
        SchroHipMotionEncodePicture & p = pics[k];
        memset (&p, 0, sizeof (p));
        unsigned long long motion, out, capacity, result;
        // (addresses only: the check dereferences nothing)
        if (fscanf (f, " p %llu %d %d %d %d %llu %llu %llu", &motion, &p.x_num_blocks, &p.y_num_blocks, &p.num_refs, &p.have_global_motion, &out,
                &capacity, &result) != 8)
          return 2;
        p.motion = (const void *) (uintptr_t) motion;
        p.out = (uint8_t *) (uintptr_t) out;
        p.capacity = (size_t) capacity;
        p.result = (SchroHipMotionEncodeResult *) (uintptr_t) result;
      }
      char message[256] = "";
      if (fscanf (f, " M %255[^\n]", message) != 1)
        message[0] = 0;
      const int r = schro_hip_motion_encode_check (pics.data (), n);
      if (refused) {
        EXPECT (r == SCHRO_HIP_EINVAL && strstr (schro_hip_last_error (), message), "%s: passes, or does not say \"%s\"", name, message);
        EXPECT (schro_hip_motion_encode_batch (ctx, pics.data (), n) == SCHRO_HIP_EINVAL, "%s: the batch runs it", name);
      } else {
        EXPECT (r == 0, "%s is refused", name);
      }
      descriptions++;
    } else {
      fprintf (stderr, "motion_enc_walk: bad table line %s\n", kind);
      return 2;
    }
  }
  fclose (f);
  // every geometry in one call
  std::vector < SchroHipMotionEncodePicture > batch;
  for (Geometry * g:geometries)
    batch.push_back (g->p);
  if (!batch.empty ())
    EXPECT (schro_hip_motion_encode_batch (ctx, batch.data (), (int) batch.size ()) == 0, "batch of %zu", batch.size ());
  if (!geometries.empty ()) {
    Geometry & g = *geometries[0];
    EXPECT (schro_hip_motion_encode_batch (nullptr, &g.p, 1) == SCHRO_HIP_EINVAL, "no context passes");
    EXPECT (schro_hip_motion_encode_check (nullptr, 1) == SCHRO_HIP_EINVAL, "no pictures pass");
    EXPECT (schro_hip_motion_encode_check (&g.p, 0) == SCHRO_HIP_EINVAL, "an empty call passes");
    EXPECT (schro_hip_motion_encode_bound (0, 4, 1, 0) == SCHRO_HIP_EINVAL, "a bound of nothing");
    EXPECT (schro_hip_encode_motion_data_noarith (nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == SCHRO_HIP_EINVAL,
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
  printf ("motion_enc_walk: %zu geometries, %d descriptions, %s\n", count, descriptions, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
