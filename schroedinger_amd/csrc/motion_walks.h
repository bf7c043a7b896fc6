// motion_walks.h -- what the three walks of a motion-data decoder are made of, shared by motion_dec.hip (VLC) and
// motion_arith_dec.hip (arithmetic): the workgroup's prefix scan, the majority of the three neighbours' flags, a unit's
// blocks and a superblock's units in stream order, and a neighbour's record as the vector and DC predictions read it.
// Moved unchanged out of motion_dec.hip; the walks themselves differ in where residuals and mode bits come from and stay
// with their files.
#pragma once

#include "motion_common.h"

namespace schro {
namespace {

// an inclusive scan over the workgroup's threads, `n` words a thread, in LDS (part: n rows of blockDim.x words)
template < int N > __device__ __forceinline__ void
md_block_scan (uint32_t * part, uint32_t mine[N])
{
  const int tid = (int) threadIdx.x, T = (int) blockDim.x;
#pragma unroll
  for (int k = 0; k < N; k++)
    part[k * T + tid] = mine[k];
  __syncthreads ();
  for (int d = 1; d < T; d <<= 1) {
    uint32_t v[N];
#pragma unroll
    for (int k = 0; k < N; k++)
      v[k] = tid >= d ? part[k * T + tid - d] : 0u;
    __syncthreads ();
#pragma unroll
    for (int k = 0; k < N; k++)
      part[k * T + tid] += v[k];
    __syncthreads ();
  }
}

// the flags of block (x, y)'s three neighbours for the mode and global predictions: left, above, above-left
__device__ __forceinline__ uint32_t
md_majority (const uint32_t * st, int nbx, int x, int y)
{
  const uint32_t a = x > 0 ? gload < uint32_t > (st + (size_t) y * nbx + x - 1) : 0u;
  const uint32_t b = y > 0 ? gload < uint32_t > (st + (size_t) (y - 1) * nbx + x) : 0u;
  const uint32_t c = x > 0 && y > 0 ? gload < uint32_t > (st + (size_t) (y - 1) * nbx + x - 1) : 0u;
  // schro_motion_get_mode_prediction, schro_motion_get_global_prediction (:402-430, :213-239): at an edge the one
  // neighbour there is; inside the majority of three, bit by bit
  return y == 0 ? a : x == 0 ? b : (a & b) | (b & c) | (c & a);
}

__device__ __forceinline__ void
md_store_unit (uint32_t * st, int nbx, int x, int y, int step, uint32_t flags)
{
  for (int l = 0; l < step; l++)
    for (int c = 0; c < step; c++)
      gstore < uint32_t > (st + (size_t) (y + l) * nbx + x + c, flags);
}

// the units of superblock sb in stream order: f (x, y)
template < class F > __device__ __forceinline__ void
md_units (int nsbx, int sb, uint32_t split, const F & f)
{
  const int sy = sb / nsbx, sx = sb - sy * nsbx, step = 4 >> split;
  for (int l = 0; l < 4; l += step)
    for (int c = 0; c < 4; c += step)
      f (4 * sx + c, 4 * sy + l);
}

// a record as prediction reads it
struct MdRec {
  uint32_t flags, dx, dy;
};

struct MdNeighbours {
  int x, y;
  MdRec left, above, diag;
  __device__ __forceinline__ bool operator () (int xx, int yy, int mode, int *vx, int *vy) const
  {
    const MdRec & r = yy == y ? left : (xx == x ? above : diag);
    return mv_predicts (r.flags, r.dx, r.dy, mode, vx, vy);
  }
};

__device__ __forceinline__ MdRec
md_load (const uint8_t * field, int nbx, int x, int y)
{
  MdRec r;
  GlobalRecords { field, nbx }.raw (x, y, &r.flags, &r.dx, &r.dy);
  return r;
}

__device__ __forceinline__ int
md_dc (const MdRec & r, int i)
{
  return i == 0 ? (int16_t) r.dx : i == 1 ? (int16_t) (r.dx >> 16) : (int16_t) r.dy;
}

}                               // namespace
}                               // namespace schro
