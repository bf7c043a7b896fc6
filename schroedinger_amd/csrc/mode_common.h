// mode_common.h -- what the two mode-decision files share (mode_split2.hip: the split-2 level alone; mode_decision.hip:
// schro_mode_decision entire): the prediction of 16 samples of a row from a tiled upsampled image, the bi-reference
// average, the entropy estimate, a motion record as five dwords, schro_motion_vector_prediction over any source of
// neighbour records, and the split-2 trial of one block (schro_do_split2's loop body, schromotionest.c:1650-1800).
// The scores are a rounded product and a rounded sum: contraction is switched off from here to the end of the including
// file (subpel.hip says why).
#pragma once

#include "schro_hip_internal.h"
#include "scan_common.h"

#pragma clang fp contract(off)

namespace schro {

constexpr int kSplit2Ints = 16;         // SCHRO_HIP_SPLIT2_TABLE_INTS
// the table entry (include/schro_hip.h)
constexpr int kT_Chroma = 0, kT_BiOk = 2, kT_BiLuma = 3, kT_BiChroma = 4, kT_Dc = 5, kT_DcError = 8, kT_Area = 9;
constexpr int kSplit2IntMax = 0x7fffffff;

static_assert (kSplit2Ints == SCHRO_HIP_SPLIT2_TABLE_INTS, "the table entry");

// 16 samples of component `cb` from half-pel column X (and every second one after it) of half-pel row Y
__device__ __forceinline__ u32x4
split2_tap (const uint8_t * up, int stride, int w, int h, int X, int Y, int pair, int cb)
{
  const int Yc = min (max (Y, 0), 2 * h - 2);
  const int xp = min (max (X >> 1, -kHpApron), w + kHpApron - 1) + kHpApron;
  const uint8_t *row = up + hp_row_offset (Yc >> 1, stride) + (size_t) (((X & 1) + 2 * (Yc & 1)) * 128);
  if (!pair)
    return gload < u32x4_u > (row + hp_col_offset (xp));
  // (U, V) pairs: 8 samples per load
  const u32x4 a = gload < u32x4_u > (row + hp_col_offset (2 * xp));
  const u32x4 b = gload < u32x4_u > (row + hp_col_offset (2 * min (xp + 8, w + 2 * kHpApron - 1)));
  const uint32_t sel = cb ? 0x07050301u : 0x06040200u;
  u32x4 v;
  v[0] = __builtin_amdgcn_perm (a[1], a[0], sel);
  v[1] = __builtin_amdgcn_perm (a[3], a[2], sel);
  v[2] = __builtin_amdgcn_perm (b[1], b[0], sel);
  v[3] = __builtin_amdgcn_perm (b[3], b[2], sel);
  return v;
}

// schro_upsampled_frame_get_block_fast_precN: 16 samples of the row whose first sample lies at (x, y) in units of mvprec
__device__ __forceinline__ u32x4
split2_predict (const uint8_t * up, int stride, int w, int h, int x, int y, int mvprec, int pair, int cb)
{
  int hx = x, hy = y, rx = 0, ry = 0;
  if (mvprec == 0) {
    hx = 2 * x, hy = 2 * y;
  } else if (mvprec == 2) {
    hx = x >> 1, rx = (x & 1) << 1;
    hy = y >> 1, ry = (y & 1) << 1;
  } else if (mvprec == 3) {
    hx = x >> 2, rx = x & 3;
    hy = y >> 2, ry = y & 3;
  }
  if ((rx | ry) == 0)
    return split2_tap (up, stride, w, h, hx, hy, pair, cb);
  const uint32_t wt[4] = { (uint32_t) ((4 - ry) * (4 - rx)), (uint32_t) ((4 - ry) * rx), (uint32_t) (ry * (4 - rx)), (uint32_t) (ry * rx) };
  u32x4 even = { 0x00080008u, 0x00080008u, 0x00080008u, 0x00080008u }, odd = even;
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (wt[t]) {
      const u32x4 s = split2_tap (up, stride, w, h, hx + (t & 1), hy + (t >> 1), pair, cb);
      even += (s & 0x00ff00ffu) * wt[t];
      odd += ((s >> 8) & 0x00ff00ffu) * wt[t];
    }
  return ((even >> 4) & 0x00ff00ffu) | (((odd >> 4) & 0x00ff00ffu) << 8);
}

// (a + b + 1) >> 1 on every byte: schro_metric_get_biref with weights 1, 1 and shift 1
__device__ __forceinline__ u32x4
split2_average (u32x4 a, u32x4 b)
{
  const u32x4 even = ((a & 0x00ff00ffu) + (b & 0x00ff00ffu) + 0x00010001u) >> 1;
  const u32x4 odd = (((a >> 8) & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu) + 0x00010001u) >> 1;
  return (even & 0x00ff00ffu) | ((odd & 0x00ff00ffu) << 8);
}

// the mask of dword d of a segment that holds `valid` samples of the block
__device__ __forceinline__ uint32_t
split2_mask (int valid, int d)
{
  const int n = min (max (valid - 4 * d, 0), 4);
  return n == 4 ? 0xffffffffu : (1u << (8 * n)) - 1;
}

__device__ __forceinline__ uint32_t
split2_wave_sum (uint32_t v)
{
  for (int off = 32; off; off >>= 1)
    v += (uint32_t) __shfl_xor ((int) v, off);
  return v;
}

// schro_pack_estimate_sint (schropack.c:204-226)
__device__ __forceinline__ int
split2_estimate_sint (int value)
{
  const uint32_t a = (uint32_t) (value < 0 ? -value : value);
  const int n_bits = 32 - __clz ((int) (a + 1));        // maxbit (value + 1)
  return n_bits + n_bits - 1 + (a ? 1 : 0);
}

__device__ __forceinline__ int
split2_median3 (int a, int b, int c)
{
  return max (min (a, b), min (max (a, b), c));
}

// a SchroMotionVector as five dwords: flags, metric, chroma_metric, dx[0] | dx[1] << 16, dy[0] | dy[1] << 16 -- or
// dc[0] | dc[1] << 16, dc[2] | (what dy[1] was) << 16
struct Split2Record {
  uint32_t w[5];
};

__device__ __forceinline__ Split2Record
split2_load (const uint8_t * p)
{
  Split2Record r;
#pragma unroll
  for (int n = 0; n < 5; n++)
    r.w[n] = gload < uint32_t > (p + 4 * n);
  return r;
}

// mv->split = 2; mv->pred_mode = mode; mv->using_global = 0
__device__ __forceinline__ uint32_t
split2_flags (uint32_t flags, int mode)
{
  return (flags & ~0x1fu) | (2u << 3) | (uint32_t) mode;
}

// The neighbours of the final field in global memory: what a block of another superblock -- and, in the split-2 stage,
// every block -- is seen as.  A source of neighbour records gives flags, dx[0] | dx[1] << 16 and dy[0] | dy[1] << 16.
struct Split2GlobalRecords {
  const uint8_t *motion;
  int nbx;
  __device__ __forceinline__ void operator () (int x, int y, uint32_t * flags, uint32_t * dx, uint32_t * dy) const
  {
    const uint8_t *mv = motion + ((size_t) y * nbx + x) * 20;
    *flags = gload < uint32_t > (mv);
    *dx = gload < uint32_t > (mv + 12);
    *dy = gload < uint32_t > (mv + 16);
  }
};

// schro_motion_vector_prediction (schromotion.c:315-368) for block (i, j), mode 1 or 2
template < class Records > __device__ __forceinline__ void
split2_vector_prediction (const Records & get, int i, int j, int mode, int *px, int *py)
{
  int vx[3], vy[3], n = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const bool there = k == 0 ? i > 0 : k == 1 ? j > 0 : i > 0 && j > 0;
    if (there) {
      uint32_t flags, dx, dy;
      get (k == 1 ? i : i - 1, k == 0 ? j : j - 1, &flags, &dx, &dy);
      if (!(flags & 4) && (flags & (uint32_t) mode)) {
        vx[n] = (int16_t) (dx >> (16 * (mode - 1)));
        vy[n++] = (int16_t) (dy >> (16 * (mode - 1)));
      }
    }
  }
  *px = 0, *py = 0;
  if (n == 1)
    *px = vx[0], *py = vy[0];
  else if (n == 2)
    *px = (vx[0] + vx[1] + 1) >> 1, *py = (vy[0] + vy[1] + 1) >> 1;
  else if (n == 3)
    *px = split2_median3 (vx[0], vx[1], vx[2]), *py = split2_median3 (vy[0], vy[1], vy[2]);
}

// one round of schro_do_split2's loops for block (i, j) inside the picture, by one lane: the record, best_error and
// best_entropy
template < class Records > __device__ __forceinline__ Split2Record
split2_block_trial (const Split2Job * jb, const Records & get, int i, int j, int *error_out, int *entropy_out)
{
  const int nbx = jb->nbx, nrefs = jb->num_refs;
  const size_t blk = (size_t) j * nbx + i;
  const int32_t *t = jb->table + blk * kSplit2Ints;
  const double lambda = jb->lambda;
  double min_score = __builtin_huge_val ();
  int entropy[2] = { 0, 0 }, best_entropy = kSplit2IntMax, best_error = kSplit2IntMax;
  Split2Record best = { {0x11u, 0, 0, 0, 0} }, mv = best, first = best;
#pragma unroll
  for (int ref = 0; ref < 2; ref++) {
    if (ref >= nrefs)
      continue;
    mv = split2_load (jb->field[ref] + blk * 20);
    if (ref == 0)
      first = mv;
    mv.w[0] = split2_flags (mv.w[0], ref + 1);
    int px, py;
    split2_vector_prediction (get, i, j, ref + 1, &px, &py);
    const int dx = (int16_t) (mv.w[3] >> (16 * ref)), dy = (int16_t) (mv.w[4] >> (16 * ref));
    entropy[ref] = split2_estimate_sint (dx - px) + split2_estimate_sint (dy - py);
    // schro_get_split2_metric
    int error = kSplit2IntMax;
    if (mv.w[1] != (uint32_t) kSplit2IntMax) {
      mv.w[2] = (uint32_t) gload < int32_t > (t + kT_Chroma + ref);
      error = (int) (mv.w[2] + mv.w[1]);
    }
    const double score = (double) entropy[ref] + (double) error * lambda;     // (not contracted: the pragma above)
    if (min_score > score) {
      min_score = score;
      best = mv;
      best_entropy = entropy[ref];
      best_error = (int) mv.w[1];
    }
  }
  int area = 0;
  if (nrefs > 1) {
    mv.w[3] = (first.w[3] & 0xffffu) | (mv.w[3] & 0xffff0000u);
    mv.w[4] = (first.w[4] & 0xffffu) | (mv.w[4] & 0xffff0000u);
    mv.w[0] = split2_flags (mv.w[0], 3);
    area = gload < int32_t > (t + kT_Area);
    if (gload < int32_t > (t + kT_BiOk)) {
      mv.w[1] = (uint32_t) gload < int32_t > (t + kT_BiLuma);
      mv.w[2] = (uint32_t) gload < int32_t > (t + kT_BiChroma);
      const double score = (double) (entropy[0] + entropy[1]) + (double) (mv.w[1] + mv.w[2]) * lambda;
      if (min_score > score) {
        best_error = (int) (mv.w[1] + mv.w[2]);
        best_entropy = entropy[0] + entropy[1];
        best = mv;
        min_score = score;
      }
    }
  }
  if (4 * area < best_error) {
    const int error = gload < int32_t > (t + kT_DcError);
    if (error != -1) {
      const int dc0 = gload < int32_t > (t + kT_Dc), dc1 = gload < int32_t > (t + kT_Dc + 1), dc2 = gload < int32_t > (t + kT_Dc + 2);
      if (error < best_error) {
        best.w[0] = split2_flags (mv.w[0], 0);
        best.w[1] = (uint32_t) error;
        best.w[2] = mv.w[2];
        best.w[3] = ((uint32_t) dc0 & 0xffffu) | ((uint32_t) dc1 << 16);
        best.w[4] = ((uint32_t) dc2 & 0xffffu) | (mv.w[4] & 0xffff0000u);
        best_error = error;
        best_entropy = split2_estimate_sint (dc0) + split2_estimate_sint (dc1) + split2_estimate_sint (dc2);
      }
    }
  }
  *error_out = best_error;
  *entropy_out = best_entropy;
  return best;
}

}                               // namespace schro
