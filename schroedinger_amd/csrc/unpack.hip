// unpack.hip -- the encoder-direction schro_frame_convert for gfx950: a packed picture (YUYV / UYVY / AYUV / v210 /
// v216 / AY64) or a planar frame -> a planar u8 / s16 / s32 frame.
//
// What it computes: what the chain of virtual frames of schro_frame_convert (schroframe.c:869-979) renders --
// schro_virt_frame_new_unpack (schrovirtframe.c:616-940), the depth step (schroframe.c:905-924), the u8 chroma
// decimation / repetition (schrovirtframe.c:1438-1576), crop or edge extension (:1823-1960) -- evaluated backwards per
// destination sample: clamp the coordinate, scale the chroma coordinate, fetch the sample from its packed row
// (unpack_fetch.h), change the depth.
//
// How: one job per (picture, component), all pictures of a call in one launch.  A lane owns one 16-byte piece of one
// destination row (16 / 8 / 4 samples); a wave covers 64 consecutive pieces of a row, so its 16-byte source loads and
// its 16-byte stores run along whole lines.  Where the destination's pointer or stride is no multiple of 16, and in a
// row's last partial piece, the samples are stored one by one.
//
// Bound: HBM.  Bytes per destination sample: the packed bytes it shares (YUYV / UYVY 2 per pixel, v210 8 / 3, AYUV 4,
// v216 4, AY64 8; rows are read once per component, the other two passes hit L2) + the sample itself.

#include "schro_hip_internal.h"
#include "unpack_fetch.h"

namespace schro {
namespace {

constexpr int kThreads = 256;
constexpr int kPiecesX = 64;    // 16-byte pieces of a row per tile: one wave
constexpr int kRows = kThreads / kPiecesX;

template < int DBPP >
__device__ __forceinline__ void
unpack_tile (const UnpackJob & job, int t, int tid)
{
  constexpr int N = 16 / DBPP;  // samples per piece
  const int ty = t / job.tiles_x;
  const int tx = t - ty * job.tiles_x;
  const int y = ty * kRows + tid / kPiecesX;
  const int x0 = (tx * kPiecesX + tid % kPiecesX) * N;
  if (y >= job.h || x0 >= job.w)
    return;

  int ys = min (y, job.ymax);
  ys = job.ysh > 0 ? ys << 1 : job.ysh < 0 ? ys >> 1 : ys;
  const uint8_t *row = job.s.base + (size_t) ys * job.s.stride;
  RowWords rw;
  rw.row = nullptr;
  rw.q = -1;
  rw.w = (u32x4) { 0, 0, 0, 0 };
  uint32_t o[4] = { 0, 0, 0, 0 };
  unpack_by_kind (job.s.kind, [&](auto kind) {
#pragma unroll
    for (int i = 0; i < N; i++) {
      int xs = min (x0 + i, job.xmax);
      xs = job.xsh > 0 ? xs << 1 : job.xsh < 0 ? xs >> 1 : xs;
      const int v = unpack_depth (unpack_sample < decltype (kind)::value > (rw, job.s, row, xs), job.s.depth, DBPP);
      if constexpr (DBPP == 1)
        o[i >> 2] |= (uint32_t) (v & 0xff) << (8 * (i & 3));
      else if constexpr (DBPP == 2)
        o[i >> 1] |= (uint32_t) (v & 0xffff) << (16 * (i & 1));
      else
        o[i] = (uint32_t) v;
    }
  });

  uint8_t *d = job.dst + (size_t) y * job.dst_stride + (size_t) x0 * DBPP;
  if (job.vec && x0 + N <= job.w) {
    gstore < u32x4 > (d, (u32x4) { o[0], o[1], o[2], o[3] });
  } else {
    // the scalar tail form
#pragma unroll
    for (int i = 0; i < N; i++)
      if (x0 + i < job.w) {
        if constexpr (DBPP == 1)
          gstore < uint8_t > (d + i, (uint8_t) (o[i >> 2] >> (8 * (i & 3))));
        else if constexpr (DBPP == 2)
          gstore < uint16_t > (d + 2 * i, (uint16_t) (o[i >> 1] >> (16 * (i & 1))));
        else
          gstore < uint32_t > (d + 4 * i, o[i]);
      }
  }
}

}                               // namespace

// (the destination depth is uniform per workgroup: a scalar switch)
__global__ __launch_bounds__ (kThreads)
void unpack_kernel (const UnpackJob * __restrict__ jobs, int njobs)
{
  const int bid = blockIdx.x;
  const UnpackJob job = jobs[find_job (jobs, njobs, bid)];
  const int t = bid - job.tile_base;
  if (job.dst_bpp == 1)
    unpack_tile < 1 > (job, t, threadIdx.x);
  else if (job.dst_bpp == 2)
    unpack_tile < 2 > (job, t, threadIdx.x);
  else
    unpack_tile < 4 > (job, t, threadIdx.x);
}

void
unpack_tile_geometry (int *pieces_x, int *rows)
{
  *pieces_x = kPiecesX;
  *rows = kRows;
}

int
launch_unpack (hipStream_t stream, const UnpackJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH (unpack_kernel, dim3 (total_tiles), dim3 (kThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "unpack launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
