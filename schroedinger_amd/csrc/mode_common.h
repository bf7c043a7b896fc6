// mode_common.h -- what the two mode-decision files share (mode_split2.hip: the split-2 level alone; mode_decision.hip:
// schro_mode_decision entire) over motion_common.h, which has the prediction of 16 samples of a row from a tiled upsampled
// image, the entropy estimate and schro_motion_vector_prediction over any source of neighbour records: the bi-reference
// average, a motion record as five dwords, and the split-2 trial of one block (schro_do_split2's loop body,
// schromotionest.c:1650-1800).
// The scores are a rounded product and a rounded sum: contraction is switched off from here to the end of the including
// file (subpel.hip says why).
#pragma once

#include "motion_common.h"

#pragma clang fp contract(off)

namespace schro {

constexpr int kSplit2Ints = 16;         // SCHRO_HIP_SPLIT2_TABLE_INTS
// the table entry (include/schro_hip.h)
constexpr int kT_Chroma = 0, kT_BiOk = 2, kT_BiLuma = 3, kT_BiChroma = 4, kT_Dc = 5, kT_DcError = 8, kT_Area = 9;
constexpr int kSplit2IntMax = 0x7fffffff;

static_assert (kSplit2Ints == SCHRO_HIP_SPLIT2_TABLE_INTS, "the table entry");

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

// a SchroMotionVector as five dwords: flags, metric, chroma_metric, dx[0] | dx[1] << 16, dy[0] | dy[1] << 16 -- or
// dc[0] | dc[1] << 16, dc[2] | (what dy[1] was) << 16
struct Split2Record {
  uint32_t w[kMvDwords];
};
static_assert (kMvFlags == 0 && kMvMetric == 4 && kMvChromaMetric == 8 && kMvDx == 12 && kMvDy == 16, "w[0] .. w[4]");

__device__ __forceinline__ Split2Record
split2_load (const uint8_t * p)
{
  Split2Record r;
#pragma unroll
  for (int n = 0; n < kMvDwords; n++)
    r.w[n] = gload < uint32_t > (p + 4 * n);
  return r;
}

__device__ __forceinline__ void
split2_store (uint8_t * p, const Split2Record & r)
{
#pragma unroll
  for (int n = 0; n < kMvDwords; n++)
    gstore < uint32_t > (p + 4 * n, r.w[n]);
}

// mv->split = 2; mv->pred_mode = mode; mv->using_global = 0
__device__ __forceinline__ uint32_t
split2_flags (uint32_t flags, int mode)
{
  return (flags & ~0x1fu) | (2u << 3) | (uint32_t) mode;
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
    mv = split2_load (jb->field[ref] + blk * kMvBytes);
    if (ref == 0)
      first = mv;
    mv.w[0] = split2_flags (mv.w[0], ref + 1);
    int px, py;
    vector_prediction (get, i, j, ref + 1, &px, &py);
    const int dx = (int16_t) (mv.w[3] >> (16 * ref)), dy = (int16_t) (mv.w[4] >> (16 * ref));
    entropy[ref] = estimate_sint (dx - px) + estimate_sint (dy - py);
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
        best_entropy = estimate_sint (dc0) + estimate_sint (dc1) + estimate_sint (dc2);
      }
    }
  }
  *error_out = best_error;
  *entropy_out = best_entropy;
  return best;
}

}                               // namespace schro
