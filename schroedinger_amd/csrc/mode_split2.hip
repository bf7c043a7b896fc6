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
//
// The prediction of a row segment (predict), the vector prediction over the final field (GlobalRecords) and the walk over
// the anti-diagonals are motion_common.h's; the trial of a block is mode_common.h's.

#include "mode_common.h"

#pragma clang fp contract(off)

namespace schro {

constexpr int kSplit2Waves = 4;
constexpr int kSplit2Threads = kSplit2Waves * 64;
constexpr int kSplit2ChooseThreads = 256;

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
  int vx0, vy0, vx1 = 0, vy1 = 0;
  mv_vector (mv_record (jb->field[0], nbx, i, j), 0, &vx0, &vy0);
  if (nrefs == 2)
    mv_vector (mv_record (jb->field[1], nbx, i, j), 1, &vx1, &vy1);
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
    pred0 = predict (jb->up[0][pair ? c : k], up_stride, tw, th, (tx << mvprec) + (vx0 >> hs), (ty << mvprec) + (vy0 >> vs), mvprec,
        k ? pair : 0, k == 2);
    if (nrefs == 2)
      pred1 = predict (jb->up[1][pair ? c : k], up_stride, tw, th, (tx << mvprec) + (vx1 >> hs), (ty << mvprec) + (vy1 >> vs), mvprec,
          k ? pair : 0, k == 2);
    if (from_v) {
      const int xv = (xo1 + 16 * a.seg) << mvprec, yv = (yo1 + a.r) << mvprec;
      other0 = predict (jb->up[0][pair ? 1 : 2], jb->up_stride[1], w1, h1, xv + (vx0 >> jb->hs), yv + (vy0 >> jb->vs), mvprec, pair, 1);
      other1 = predict (jb->up[1][pair ? 1 : 2], jb->up_stride[1], w1, h1, xv + (vx1 >> jb->hs), yv + (vy1 >> jb->vs), mvprec, pair, 1);
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

// one round of schro_do_split2's loops for block (i, j) inside the picture, by one lane (mode_common.h)
__device__ __forceinline__ void
split2_choose_block (const Split2Job * jb, int i, int j)
{
  const int nbx = jb->nbx;
  const GlobalRecords get = { jb->motion, nbx };
  int best_error, best_entropy;
  split2_store (mv_record (jb->motion, nbx, i, j), split2_block_trial (jb, get, i, j, &best_error, &best_entropy));
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
    if (i >= cols || j >= rws)
      split2_store (mv_record (jb->motion, nbx, i, j), Split2Record { {0x11u, 0, 0, 0, 0} });
  }
  __threadfence ();
  __syncthreads ();
  walk_diagonals (cols, rws, (int) threadIdx.x, (int) blockDim.x, [&](int i, int j) {
        split2_choose_block (jb, i, j);
      });
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
