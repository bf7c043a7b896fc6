// plane_iwt.cpp -- the C ABI of libschro_hip.so (include/schro_hip.h), plane layer: the forward wavelet
// (schro_hip_iwt_batch: the level loop of schro_frame_iwt_transform / schro_gpuframe_iwt_transform over iwt_fwd.hip's
// level kernel, finest level first).

#include "schro_hip_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

using namespace schro;

namespace schro {

int
iwt_batch_run (SchroHipContext * ctx, const SchroHipIwtFwdPlane * planes, int nplanes, int depth, int filter, int bpp,
    bool in_place, const IwtFwdPacked * packed)
{
  SCHRO_HIP_REQUIRE (ctx && planes && nplanes > 0, "iwt_batch: bad arguments");
  SCHRO_HIP_REQUIRE (nplanes <= kMaxJobs, "iwt_batch: at most %d planes per call", kMaxJobs);
  SCHRO_HIP_REQUIRE (depth >= 1 && depth <= 6, "iwt_batch: transform depth %d out of range", depth);
  SCHRO_HIP_REQUIRE (filter >= 0 && filter <= 6, "iwt_batch: wavelet filter index %d out of range", filter);
  SCHRO_HIP_REQUIRE (bpp == 2 || bpp == 4, "iwt_batch: bytes_per_sample must be 2 or 4");
  (void) hipSetDevice (ctx->device);

  int uc, ur;
  iwt_fwd_tile_geometry (filter, bpp, &uc, &ur);

  // the scratch: (in place) a copy of every source plane, then the LL images of levels 0 .. depth - 2 of every plane
  std::vector < size_t > copy_off (nplanes, 0), ll_off ((size_t) nplanes * depth, 0);
  std::vector < int >copy_stride (nplanes, 0), ll_stride ((size_t) nplanes * depth, 0);
  size_t total = 0;
  for (int p = 0; p < nplanes; p++) {
    const SchroHipIwtFwdPlane & pl = planes[p];
    const bool from_packed = packed && packed[p].packed;        // level 0 reads packed rows: no source plane
    SCHRO_HIP_REQUIRE ((pl.src || from_packed) && pl.dst, "iwt_batch: plane %d has a NULL pointer", p);
    SCHRO_HIP_REQUIRE (pl.width > 0 && pl.height > 0 && pl.width % (1 << depth) == 0 && pl.height % (1 << depth) == 0,
        "iwt_batch: plane %d size %dx%d is not a multiple of 2^depth", p, pl.width, pl.height);
    SCHRO_HIP_REQUIRE (pl.width <= (1 << 17) && pl.height <= (1 << 17), "iwt_batch: plane %d size %dx%d is too large", p, pl.width,
        pl.height);
    SCHRO_HIP_REQUIRE ((from_packed || pl.src_stride >= pl.width * bpp) && pl.dst_stride >= pl.width * bpp,
        "iwt_batch: plane %d stride too small", p);
    SCHRO_HIP_REQUIRE ((from_packed || (pl.src_stride % bpp == 0 && (uintptr_t) pl.src % bpp == 0)) && pl.dst_stride % bpp == 0
        && (uintptr_t) pl.dst % bpp == 0, "iwt_batch: plane %d: pointers and strides must be multiples of the sample size %d", p, bpp);
    if (from_packed) {
      // (plane_unpack.cpp has checked the packed rows against dst)
    } else if (!in_place) {
      const char *s0 = (const char *) pl.src, *s1 = s0 + (size_t) pl.src_stride * pl.height;
      const char *d0 = (const char *) pl.dst, *d1 = d0 + (size_t) pl.dst_stride * pl.height;
      SCHRO_HIP_REQUIRE (s1 <= d0 || d1 <= s0, "iwt_batch: plane %d src and dst overlap", p);
    } else {
      copy_stride[p] = (int) round_up ((size_t) pl.width * bpp, 128);
      copy_off[p] = total;
      total += round_up ((size_t) copy_stride[p] * pl.height, 256);
    }
    for (int l = 0; l < depth - 1; l++) {
      const int w = pl.width >> (l + 1), h = pl.height >> (l + 1);
      const int stride = (int) round_up ((size_t) w * bpp, 128);
      ll_off[(size_t) p * depth + l] = total;
      ll_stride[(size_t) p * depth + l] = stride;
      total += round_up ((size_t) stride * h, 256);
    }
  }
  if (total) {
    int r = ensure_scratch (ctx, total);
    if (r)
      return r;
  }
  char *scratch = (char *) ctx->scratch_ref ();
  if (in_place)
    for (int p = 0; p < nplanes; p++) {
      const SchroHipIwtFwdPlane & pl = planes[p];
      int r = copy_2d_async (ctx, scratch + copy_off[p], copy_stride[p], pl.src, pl.src_stride, pl.width * bpp, pl.height,
          hipMemcpyDeviceToDevice);
      if (r)
        return r;
    }

  // level 0 is two launches where planes read packed rows: theirs (pjobs) and the others'
  std::vector < IwtFwdJob > jobs;
  std::vector < IwtFwdPackedJob > pjobs;
  for (int level = 0; level < depth; level++) {
    int tile_base = 0, ptile_base = 0;
    jobs.clear ();
    pjobs.clear ();
    for (int p = 0; p < nplanes; p++) {
      const SchroHipIwtFwdPlane & pl = planes[p];
      const bool from_packed = level == 0 && packed && packed[p].packed;
      IwtFwdPackedJob pj;
      memset (&pj, 0, sizeof (pj));
      IwtFwdJob & j = pj;
      int &tile_base_of = from_packed ? ptile_base : tile_base;
      const int w = pl.width >> level, h = pl.height >> level;
      if (level > 0) {
        j.src = scratch + ll_off[(size_t) p * depth + level - 1];
        j.src_stride = ll_stride[(size_t) p * depth + level - 1];
      } else if (in_place) {
        j.src = scratch + copy_off[p];
        j.src_stride = copy_stride[p];
      } else {
        j.src = pl.src;
        j.src_stride = pl.src_stride;
      }
      // the level view of the coefficient frame {w, h, stride << level}: even rows [LL | HL], odd rows [LH | HH]
      // (schroparams.c:319-352); the LL band of every level but the last is the next level's input: to the scratch
      char *base = (char *) pl.dst;
      const int vstride = pl.dst_stride << level;
      j.band[0] = base;
      j.band_stride[0] = vstride * 2;
      if (level < depth - 1) {
        j.band[0] = scratch + ll_off[(size_t) p * depth + level];
        j.band_stride[0] = ll_stride[(size_t) p * depth + level];
      }
      j.band[1] = base + (size_t) (w / 2) * bpp;
      j.band[2] = base + vstride;
      j.band[3] = base + vstride + (size_t) (w / 2) * bpp;
      j.band_stride[1] = j.band_stride[2] = j.band_stride[3] = vstride * 2;
      j.w = w;
      j.h = h;
      const int nc = w / 2, nr = h / 2;
      const int pl_pairs = 4 / bpp;     // column pairs per 8-byte load
      const bool src_al = from_packed || (nc % pl_pairs == 0 && (((uintptr_t) j.src | (uintptr_t) j.src_stride) & 7) == 0);
      bool dst_al = nc % 4 == 0;
      for (int b = 0; b < 4; b++)
        dst_al = dst_al && (((uintptr_t) j.band[b] | (uintptr_t) j.band_stride[b]) & (size_t) (4 * bpp - 1)) == 0;
      j.flags = (src_al ? 1 : 0) | (dst_al ? 2 : 0);
      j.tiles_x = div_up (nc, uc);
      j.m_tiles_x = div_magic (j.tiles_x);
      j.tile_base = tile_base_of;
      // (the kernel's t / tiles_x is one multiply, schro_hip_internal.h mdiv: exact for tiles_x <= 1024 and fewer than
      // 2^22 tiles, which the size limit above keeps)
      tile_base_of += j.tiles_x * div_up (nr, ur);
      if (from_packed) {
        pj.s = packed[p].s;
        pj.xmax = packed[p].xmax;
        pj.ymax = packed[p].ymax;
        pjobs.push_back (pj);
      } else {
        jobs.push_back (j);
      }
    }
    ProfileScope ps (ctx, level == 0 ? SCHRO_HIP_KERNEL_IIWT_FINEST : SCHRO_HIP_KERNEL_IIWT_COARSE);
    void *d_jobs;
    if (!pjobs.empty ()) {
      int r = push_args (ctx, pjobs.data (), sizeof (IwtFwdPackedJob) * pjobs.size (), &d_jobs);
      if (r)
        return r;
      r = launch_iwt_fwd_packed (ctx->stream, (const IwtFwdPackedJob *) d_jobs, (int) pjobs.size (), ptile_base, filter, bpp);
      if (r)
        return r;
    }
    if (!jobs.empty ()) {
      int r = push_args (ctx, jobs.data (), sizeof (IwtFwdJob) * jobs.size (), &d_jobs);
      if (r)
        return r;
      r = launch_iwt_fwd_level (ctx->stream, (const IwtFwdJob *) d_jobs, (int) jobs.size (), tile_base, filter, bpp);
      if (r)
        return r;
    }
  }
  return 0;
}

}                               // namespace schro

extern "C" {

int
schro_hip_iwt_batch (SchroHipContext * ctx, const SchroHipIwtFwdPlane * planes, int nplanes, int depth, int filter,
    int bytes_per_sample)
{
  return iwt_batch_run (ctx, planes, nplanes, depth, filter, bytes_per_sample, false);
}

}                               // extern "C"
