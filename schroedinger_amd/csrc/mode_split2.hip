// mode_split2.hip -- the split-2 level of schro_mode_decision (schromotionest.c:2587-2688): schro_do_split2 (:1600-1807)
// for every superblock, then schro_motion_copy_to.  include/schro_hip.h restates the level and lays the table out.
//
// As in subpel.hip only the CHOICE is serial: a block's entropy estimate predicts its vectors from the records to the
// left, above and above-left as the level has already decided them.  Everything that reads a picture -- the chroma SADs
// of schro_get_split2_metric, the bi-reference metric over three components, the DC averages -- depends on the pictures
// and the block's own two sub-pel records alone.  So
//   * split2_metric_kernel runs over the blocks of ALL pictures on the whole device and leaves kSplit2Ints int32 per
//     block;
//   * split2_choose_kernel, one workgroup per picture, walks the anti-diagonals of the block grid with one LANE per block:
//     integer and double arithmetic on that entry and on five dwords per record, no picture is touched.
//
// split2_metric_kernel: one wave per block, kSplit2Waves blocks per workgroup, a picture's workgroups found through
// tile_base.  The block is cut into TASKS of one row segment -- up to 16 samples of one row of one component -- and a lane
// takes tasks lane, lane + 64, ..: 32 x 32 at 4:4:4 is 192 of them, 4 x 4 at 4:2:0 is 8.  A task fetches its source samples
// as four dwords (scan_fetch4: clamped to the component), masks them to the clipped block, and predicts the same 16
// samples from each reference by subpel.hip's bilinear form: half-pel origin hx, hy and eighth-pel remainder rx, ry
// (precision 0: hx = 2 x; 1: hx = x; 2: x >> 1 and 2 (x & 1); 3: x >> 2 and x & 3), a tap's 16 columns are ONE byte-aligned
// 16-byte load of the tiled image (a row of a 32-wide block is two tasks, so two loads), a tap of weight 0 is not fetched,
// v_sad_u8 takes the dwords.  A 2-sample chroma row is the same load with 14 samples masked off.  A frame's (U, V) pair
// image gives 8 samples of both components per load: two loads and a v_perm_b32 per dword.  Rows are clamped to
// [0, 2 h - 2] and then select their plane, columns are clamped to the image's aprons: no address leaves an image,
// whatever the vector (the header's REACH says which vectors the reference itself can read).
//
// The bi-reference trial at mv_precision 2 and 3 measures what the reference measures: its two fetch buffers (one per
// reference, schromotionest.c:2600-2609) receive luma, then U, then V before any metric is taken (:1698-1747), so luma is
// compared with V's prediction in its top-left width[2] x height[2] samples and U with V's prediction.  A luma task whose
// segment touches that corner predicts V's row as well and takes its bytes; a U task predicts V's row.
//
// The DC average needs the block's sums first: the wave reduces them, then walks the tasks once more for the error.
//
// split2_choose_kernel: `score = entropy + error * lambda` is a rounded product, then a rounded sum, as the reference's
// x86-64 build has it; contraction is switched off for this file by the pragma below (subpel.hip says why).  A block whose
// origin lies outside the picture takes no part in the walk: its final record is the constant best_mv, and no block inside
// the picture has such a neighbour (i * xbsep < width implies (i - 1) * xbsep < width), so the record the reference keeps
// for it while its superblock is worked on reaches only other outside records and never the result.

#include "schro_hip_internal.h"
#include "scan_common.h"

#pragma clang fp contract(off)

namespace schro {

constexpr int kSplit2Waves = 4;
constexpr int kSplit2Threads = kSplit2Waves * 64;
constexpr int kSplit2ChooseThreads = 256;
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

struct Split2Task {
  int k, r, seg;
};

// task t of a block of s0 x h0 luma and sc x hc chroma row segments
__device__ __forceinline__ Split2Task
split2_task (int t, int s0, int h0, int sc, int hc)
{
  Split2Task a;
  const int t0 = s0 * h0, tc = sc * hc;
  a.k = t < t0 ? 0 : (t < t0 + tc ? 1 : 2);
  const int u = t - (a.k ? t0 + (a.k - 1) * tc : 0), s = a.k ? sc : s0;
  a.r = s == 2 ? u >> 1 : u;
  a.seg = s == 2 ? u & 1 : 0;
  return a;
}

__global__ __launch_bounds__ (kSplit2Threads)
void split2_metric_kernel (const Split2Job * __restrict__ jobs, int njobs)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Split2Job *jb = jobs + find_job (jobs, njobs, (int) blockIdx.x);
  const int nbx = jb->nbx;
  const int blk = ((int) blockIdx.x - jb->tile_base) * kSplit2Waves + wave;
  if (blk >= nbx * jb->nby)     // (wave-uniform; the kernel has no workgroup barrier)
    return;
  const int j = blk / nbx, i = blk - j * nbx;
  int32_t *out = jb->table + (size_t) blk * kSplit2Ints;
  const int mvprec = jb->prec, nrefs = jb->num_refs, pair = jb->pair;
  // the components (0: luma, 1: either chroma): size, block, the block's origin and clipped size
  const int w0 = jb->w, h0 = jb->h, w1 = jb->cw, h1 = jb->ch;
  const int bx0 = jb->xb, by0 = jb->yb, bx1 = jb->xb >> jb->hs, by1 = jb->yb >> jb->vs;
  if (i * bx0 >= w0 || j * by0 >= h0) {        // outside the picture: no source block, SCHRO_METRIC_INVALID_2
    if (lane < kSplit2Ints)
      gstore < int32_t > (out + lane, lane == kT_Chroma || lane == kT_Chroma + 1 || lane == kT_DcError ? -1 : 0);
    return;
  }
  const int xo0 = i * bx0, yo0 = j * by0, xo1 = i * bx1, yo1 = j * by1;
  const int bw0 = min (bx0, w0 - xo0), bh0 = min (by0, h0 - yo0);
  const int bw1 = max (min (bx1, w1 - xo1), 0), bh1 = max (min (by1, h1 - yo1), 0);
  // the vectors: dx[0], dy[0] of field 0 and dx[1], dy[1] of field 1
  const uint8_t *rec0 = jb->field[0] + (size_t) blk * 20;
  const int vx0 = gload < int16_t > (rec0 + 12), vy0 = gload < int16_t > (rec0 + 16);
  int vx1 = 0, vy1 = 0;
  if (nrefs == 2) {
    const uint8_t *rec1 = jb->field[1] + (size_t) blk * 20;
    vx1 = gload < int16_t > (rec1 + 14), vy1 = gload < int16_t > (rec1 + 18);
  }
  // the bi-reference trial's admissibility: luma, the clipped block, the unscaled extension
  bool bi = nrefs == 2;
#pragma unroll
  for (int ref = 0; ref < 2; ref++) {
    const int x = i * (bx0 << mvprec) + (ref ? vx1 : vx0), y = j * (by0 << mvprec) + (ref ? vy1 : vy0);
    if (-jb->ext > x || -jb->ext > y || !((w0 << mvprec) + jb->ext > x + bw0 - 1) || !((h0 << mvprec) + jb->ext > y + bh0 - 1))
      bi = false;
  }
  const bool shared = mvprec > 1;       // the reference's fetch buffers are one per reference, not one per component
  const int s0 = (bw0 + 15) >> 4, sc = (bw1 + 15) >> 4;
  const int ntasks = s0 * bh0 + 2 * sc * bh1;

  uint32_t sum0 = 0, sum1 = 0, sum2 = 0, chroma0 = 0, chroma1 = 0, bi_luma = 0, bi_chroma = 0;
  for (int t = lane; t < ntasks; t += 64) {
    const Split2Task a = split2_task (t, s0, bh0, sc, bh1);
    const int k = a.k, c = k ? 1 : 0;
    const int tw = k ? w1 : w0, th = k ? h1 : h0, tx = (k ? xo1 : xo0) + 16 * a.seg, ty = (k ? yo1 : yo0) + a.r;
    const int valid = (k ? bw1 : bw0) - 16 * a.seg;
    const int hs = k ? jb->hs : 0, vs = k ? jb->vs : 0;
    const uint8_t *plane = jb->src[k];
    const int stride = jb->src_stride[k];
    uint32_t src[4], mask[4], s = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      mask[d] = split2_mask (valid, d);
      src[d] = mask[d] ? scan_fetch4 (plane, stride, tw, th, tx + 4 * d, ty) & mask[d] : 0;
      s = __builtin_amdgcn_sad_u8 (src[d], 0, s);
    }
    sum0 += k == 0 ? s : 0;
    sum1 += k == 1 ? s : 0;
    sum2 += k == 2 ? s : 0;
    if (!k && !bi)
      continue;
    // the row of each reference, in the units of mvprec: sample (+ c, + r) lies at (+ c << mvprec, + r << mvprec)
    const bool corner = shared && k == 0 && a.r < bh1 && 16 * a.seg < bw1;      // V's prediction lies over this segment
    const bool from_v = bi && (corner || (shared && k == 1));
    const int up_stride = jb->up_stride[c];
    u32x4 pred0, pred1 = { 0, 0, 0, 0 }, other0 = pred1, other1 = pred1;
    pred0 = split2_predict (jb->up[0][pair ? c : k], up_stride, tw, th, (tx << mvprec) + (vx0 >> hs), (ty << mvprec) + (vy0 >> vs), mvprec,
        k ? pair : 0, k == 2);
    if (nrefs == 2)
      pred1 = split2_predict (jb->up[1][pair ? c : k], up_stride, tw, th, (tx << mvprec) + (vx1 >> hs), (ty << mvprec) + (vy1 >> vs), mvprec,
          k ? pair : 0, k == 2);
    if (from_v) {
      const int xv = (xo1 + 16 * a.seg) << mvprec, yv = (yo1 + a.r) << mvprec;
      other0 = split2_predict (jb->up[0][pair ? 1 : 2], jb->up_stride[1], w1, h1, xv + (vx0 >> jb->hs), yv + (vy0 >> jb->vs), mvprec, pair, 1);
      other1 = split2_predict (jb->up[1][pair ? 1 : 2], jb->up_stride[1], w1, h1, xv + (vx1 >> jb->hs), yv + (vy1 >> jb->vs), mvprec, pair, 1);
    }
    if (k) {
#pragma unroll
      for (int d = 0; d < 4; d++) {
        chroma0 = __builtin_amdgcn_sad_u8 (pred0[d] & mask[d], src[d], chroma0);
        chroma1 = __builtin_amdgcn_sad_u8 (pred1[d] & mask[d], src[d], chroma1);
      }
    }
    if (bi) {
      u32x4 both = split2_average (pred0, pred1);
      if (shared && k == 1) {
        both = split2_average (other0, other1);
      } else if (corner) {
        const u32x4 v = split2_average (other0, other1);
        const int nv = bw1 - 16 * a.seg;        // V's samples of this segment
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const uint32_t m = split2_mask (nv, d);
          both[d] = (v[d] & m) | (both[d] & ~m);
        }
      }
      uint32_t acc = 0;
#pragma unroll
      for (int d = 0; d < 4; d++)
        acc = __builtin_amdgcn_sad_u8 (both[d] & mask[d], src[d], acc);
      bi_chroma += k ? acc : 0;
      bi_luma += k ? 0 : acc;
    }
  }
  sum0 = split2_wave_sum (sum0);
  sum1 = split2_wave_sum (sum1);
  sum2 = split2_wave_sum (sum2);
  chroma0 = split2_wave_sum (chroma0);
  chroma1 = split2_wave_sum (chroma1);
  bi_luma = split2_wave_sum (bi_luma);
  bi_chroma = split2_wave_sum (bi_chroma);

  // schro_block_average: ave = (sum + n / 2) / n, then the error against it
  const uint32_t n0 = (uint32_t) (bw0 * bh0), n1 = (uint32_t) (bw1 * bh1);
  const bool dc_ok = n0 && n1;
  const uint32_t ave0 = n0 ? (sum0 + n0 / 2) / n0 : 0, ave1 = n1 ? (sum1 + n1 / 2) / n1 : 0, ave2 = n1 ? (sum2 + n1 / 2) / n1 : 0;
  uint32_t dc_error = 0;
  for (int t = lane; t < ntasks; t += 64) {
    const Split2Task a = split2_task (t, s0, bh0, sc, bh1);
    const int k = a.k;
    const int tw = k ? w1 : w0, th = k ? h1 : h0, tx = (k ? xo1 : xo0) + 16 * a.seg, ty = (k ? yo1 : yo0) + a.r;
    const int valid = (k ? bw1 : bw0) - 16 * a.seg;
    const uint32_t flat = (k == 0 ? ave0 : k == 1 ? ave1 : ave2) * 0x01010101u;
    const uint8_t *plane = jb->src[k];
    const int stride = jb->src_stride[k];
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t m = split2_mask (valid, d);
      if (m)
        dc_error = __builtin_amdgcn_sad_u8 (scan_fetch4 (plane, stride, tw, th, tx + 4 * d, ty) & m, flat & m, dc_error);
    }
  }
  dc_error = split2_wave_sum (dc_error);

  if (lane < kSplit2Ints) {
    int32_t v = 0;
    if (lane == kT_Chroma)
      v = (int32_t) chroma0;
    else if (lane == kT_Chroma + 1)
      v = nrefs == 2 ? (int32_t) chroma1 : -1;
    else if (lane == kT_BiOk)
      v = bi;
    else if (lane == kT_BiLuma)
      v = bi ? (int32_t) bi_luma : 0;
    else if (lane == kT_BiChroma)
      v = bi ? (int32_t) bi_chroma : 0;
    else if (lane >= kT_Dc && lane < kT_Dc + 3)
      v = dc_ok ? (int32_t) (lane == kT_Dc ? ave0 : lane == kT_Dc + 1 ? ave1 : ave2) - 128 : 0;
    else if (lane == kT_DcError)
      v = dc_ok ? (int32_t) dc_error : -1;
    else if (lane == kT_Area)
      v = nrefs == 2 ? bw0 * bh0 + 2 * bw1 * bh1 : 0;
    gstore < int32_t > (out + lane, v);
  }
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

// schro_motion_vector_prediction (schromotion.c:315-368) for block (i, j) of the records at `rec`, mode 1 or 2
__device__ __forceinline__ void
split2_vector_prediction (const uint8_t * rec, int nbx, int i, int j, int mode, int *px, int *py)
{
  int vx[3], vy[3], n = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const bool there = k == 0 ? i > 0 : k == 1 ? j > 0 : i > 0 && j > 0;
    if (there) {
      const uint8_t *mv = rec - (k == 0 ? 20 : k == 1 ? (size_t) nbx * 20 : (size_t) (nbx + 1) * 20);
      const uint32_t flags = gload < uint32_t > (mv);
      if (!(flags & 4) && (flags & (uint32_t) mode)) {
        vx[n] = gload < int16_t > (mv + 12 + 2 * (mode - 1));
        vy[n++] = gload < int16_t > (mv + 16 + 2 * (mode - 1));
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

// one round of schro_do_split2's loops for block (i, j) inside the picture, by one lane
__device__ __forceinline__ void
split2_choose_block (const Split2Job * jb, int i, int j)
{
  const int nbx = jb->nbx, nrefs = jb->num_refs;
  const size_t blk = (size_t) j * nbx + i;
  uint8_t *rec = jb->motion + blk * 20;
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
    split2_vector_prediction (rec, nbx, i, j, ref + 1, &px, &py);
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
#pragma unroll
  for (int n = 0; n < 5; n++)
    gstore < uint32_t > (rec + 4 * n, best.w[n]);
  int32_t *sb = (int32_t *) (jb->sb + ((size_t) (j >> 2) * (nbx >> 2) + (i >> 2)) * 16);
  atomicAdd (sb, best_error);
  atomicAdd (sb + 1, best_entropy);
}

__global__ __launch_bounds__ (kSplit2ChooseThreads)
void split2_choose_kernel (const Split2Job * __restrict__ jobs)
{
  const Split2Job *jb = jobs + blockIdx.x;
  const int nbx = jb->nbx, nby = jb->nby, nsb = (nbx >> 2) * (nby >> 2);
  // the blocks whose origin lies inside the picture
  const int cols = min (nbx, (jb->w + jb->xb - 1) / jb->xb), rws = min (nby, (jb->h + jb->yb - 1) / jb->yb);
  // the sums start at the outside blocks' share: total_entropy += 2 each
  for (int s = (int) threadIdx.x; s < nsb; s += (int) blockDim.x) {
    const int sy = s / (nbx >> 2), sx = s - sy * (nbx >> 2);
    const int in = max (min (cols - 4 * sx, 4), 0) * max (min (rws - 4 * sy, 4), 0);
    int32_t *sb = (int32_t *) (jb->sb + (size_t) s * 16);
    gstore < int32_t > (sb, 0);
    gstore < int32_t > (sb + 1, 2 * (16 - in));
  }
  // ... and their records are the constant best_mv: split 2, pred_mode 1, everything else 0
  for (int n = (int) threadIdx.x; n < nbx * nby; n += (int) blockDim.x) {
    const int j = n / nbx, i = n - j * nbx;
    if (i >= cols || j >= rws) {
      uint8_t *rec = jb->motion + (size_t) n * 20;
#pragma unroll
      for (int k = 0; k < 5; k++)
        gstore < uint32_t > (rec + 4 * k, k ? 0u : 0x11u);
    }
  }
  __threadfence ();
  __syncthreads ();
  for (int d = 0; d < cols + rws - 1; d++) {
    const int jlo = max (0, d - (cols - 1)), jhi = min (d, rws - 1);
    for (int j = jlo + (int) threadIdx.x; j <= jhi; j += (int) blockDim.x)
      split2_choose_block (jb, d - j, j);
    __syncthreads ();           // the next diagonal reads this one's records
  }
  __threadfence ();
  __syncthreads ();
  // block->score = total_entropy + lambda * total_error
  const double lambda = jb->lambda;
  for (int s = (int) threadIdx.x; s < nsb; s += (int) blockDim.x) {
    int32_t *sb = (int32_t *) (jb->sb + (size_t) s * 16);
    const int error = atomicAdd (sb, 0), entropy = atomicAdd (sb + 1, 0);       // (the sums were made in L2)
    gstore < double >((double *) (sb + 2), (double) entropy + lambda * (double) error);
  }
}

int
split2_metric_blocks ()
{
  return kSplit2Waves;
}

int
launch_split2_metric (hipStream_t stream, const Split2Job * d_jobs, int njobs, int total_groups)
{
  if (njobs <= 0 || total_groups <= 0)
    return set_error (SCHRO_HIP_EINVAL, "split-2 metric launch: %d pictures, %d workgroups", njobs, total_groups);
  SCHRO_LAUNCH (split2_metric_kernel, dim3 (total_groups), dim3 (kSplit2Threads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "split-2 metric launch: %s", hipGetErrorString (e));
  return 0;
}

int
launch_split2_choose (hipStream_t stream, const Split2Job * d_jobs, int njobs)
{
  if (njobs <= 0)
    return set_error (SCHRO_HIP_EINVAL, "split-2 choice launch: %d pictures", njobs);
  SCHRO_LAUNCH (split2_choose_kernel, dim3 (njobs), dim3 (kSplit2ChooseThreads), 0, stream, d_jobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "split-2 choice launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
