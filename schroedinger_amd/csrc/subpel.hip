// subpel.hip -- sub-pel motion refinement, schro_encoder_motion_predict_subpel_deep (schromotionest.c:246-354): per
// precision pass an error launch and a choice launch.  include/schro_hip.h restates the function and the block fetch.
//
// Only the CHOICE of the reference's loop is serial -- the prediction of a block's vector comes from the records to the
// left, above and above-left as the pass has already refined them.  The eight errors of a block, and which of the eight
// candidates are admissible, depend on nothing but the block's own vector at the start of the pass.  So
//   * subpel_error_kernel runs over the blocks of ALL chains on the whole device and leaves eight int32 per block: the
//     SAD of an admissible candidate, -1 for an inadmissible one, eight times -1 for a skipped block;
//   * subpel_choose_kernel, one workgroup per chain, walks the anti-diagonals of the block grid with one LANE per block:
//     integer and double arithmetic on those eight numbers, no picture is touched.
// (hier_bm.hip has the SADs inside the chain: DESIGN 4.12 says what that costs.)
//
// subpel_error_kernel: one wave per block, kSubpelWaves blocks per workgroup, a chain's workgroups found through
// tile_base as the other batches find theirs.  The wave stages the clipped source block in its LDS once.  Lane = candidate
// k (lane & 7) x row group (lane >> 3): the lane takes rows rg, rg + 8, .. of candidate k.  All three precisions are ONE
// form: with hx, hy the half-pel origin and rx, ry the eighth-pel remainder (precision 1: remainder 0; precision 2: x >>
// 1 and 2 * (x & 1)) a sample is (w00 S (hx, hy) + w01 S (hx + 1, hy) + w10 S (hx, hy + 1) + w11 S (hx + 1, hy + 1) + 8)
// >> 4 with the bilinear weights, which sum to 16 -- weight 16 is the sample itself, 8 + 8 is avgub, no sum passes 4088:
// nothing saturates.  A tap of weight 0 is not fetched.  The tiled image keeps any run of up to 17 columns of a plane row
// inside one 32-byte chunk: a tap's 16 columns are ONE byte-aligned 16-byte load (blocks over 16 wide: two), the weights
// are applied to the even and the odd bytes of a dword as two 16-bit halves each, v_sad_u8 takes the dword.  The half-pel
// row is clamped to [0, 2 h - 2] (the image has no row aprons) and THEN selects its plane; the column is what the host
// has checked (the header's REACH) and is clamped to the image's aprons all the same: no address leaves the image.
//
// subpel_choose_kernel: `score = entropy + lambda * error` is a rounded product, then a rounded sum, as the reference's
// x86-64 build has it.  hipcc would contract the two into an FMA, and that changes decisions (lambda 0.1: entropy 27,
// metric 2557 against entropy 25, error 2577); contraction is switched off for this file by the pragma below.
//
// The tap fetch and the bilinear form (predict_halfpel), the entropy estimate, the vector prediction and the walk over the
// anti-diagonals are motion_common.h's, shared with the mode decision.

#include "motion_common.h"

#pragma clang fp contract(off)

namespace schro {

constexpr int kSubpelWaves = 4;
constexpr int kSubpelThreads = kSubpelWaves * 64;
constexpr int kSubpelChooseThreads = 256;
constexpr int kSubpelMaxBlock = 32;

// the vector of a record after `mv->u.vec.dx[ref] <<= 1` on an int16_t, and dy likewise
__device__ __forceinline__ void
subpel_doubled (const uint8_t * rec, int ref, int *dx, int *dy)
{
  mv_vector (rec, ref, dx, dy);
  *dx = (int16_t) ((uint32_t) * dx << 1);
  *dy = (int16_t) ((uint32_t) * dy << 1);
}

// offset k of sp_matches (schromotionest.c:259-262)
__device__ __forceinline__ void
subpel_offset (int k, int *ox, int *oy)
{
  const int kk = k < 4 ? k : k + 1;     // the centre is not among them
  const int q = kk >= 6 ? 2 : (kk >= 3 ? 1 : 0);
  *ox = kk - 3 * q - 1;
  *oy = q - 1;
}

__global__ __launch_bounds__ (kSubpelThreads)
void subpel_error_kernel (const SubpelChain * __restrict__ chains, int nchains, int mvprec)
{
  __shared__ __attribute__ ((aligned (16))) uint32_t subpel_lds[kSubpelWaves][kSubpelMaxBlock * kSubpelMaxBlock / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SubpelChain *ch = chains + find_job (chains, nchains, (int) blockIdx.x);
  const int nbx = ch->nbx, xb = ch->xb, yb = ch->yb, w = ch->w, h = ch->h;
  const int blk = ((int) blockIdx.x - ch->tile_base) * kSubpelWaves + wave;
  if (blk >= nbx * ch->nby)     // (wave-uniform; the kernel has no workgroup barrier)
    return;
  const int j = blk / nbx, i = blk - j * nbx;
  int32_t *out = ch->table + (size_t) blk * 8;
  const int x0 = i * xb, y0 = j * yb;
  if (x0 >= w || y0 >= h) {     // schro_frame_get_data fails: skipped
    if (lane < 8)
      gstore < int32_t > (out + lane, -1);
    return;
  }
  const int bw = min (xb, w - x0), bh = min (yb, h - y0);
  const int nd = (bw + 3) >> 2;
  const uint32_t tail = scan_tail_mask (bw);
  uint32_t *block = subpel_lds[wave];
  scan_stage_block (block, ch->src, ch->src_stride, w, h, x0, y0, nd, bh, tail, lane);
  wave_sync ();

  int dx, dy;
  subpel_doubled (mv_record (ch->field, nbx, i, j), ch->ref, &dx, &dy);
  const int k = lane & 7, rg = lane >> 3;
  int ox, oy;
  subpel_offset (k, &ox, &oy);
  const int x = i * (xb << mvprec) + dx + ox, y = j * (yb << mvprec) + dy + oy;
  const int ext = ch->ext;
  const bool ok = -ext < x && (w << mvprec) + ext > x + xb - 1 && -ext < y && (h << mvprec) + ext > y + yb - 1;
  // the half-pel origin and the remainder in eighths
  int hx, hy, rx, ry;
  halfpel_split (x, y, mvprec, &hx, &hy, &rx, &ry);
  const uint8_t *up = ch->up;
  const int stride = ch->up_stride;
  uint32_t acc = 0;
  if (ok) {
    for (int r = rg; r < bh; r += 8) {
      const uint32_t *brow = block + r * nd;
      for (int seg = 0; seg * 4 < nd; seg++) {
        const u32x4 v = predict_halfpel (up, stride, w, h, hx + 32 * seg, hy + 2 * r, rx, ry, 0, 0);
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const int n = seg * 4 + d;
          if (n < nd)
            acc = __builtin_amdgcn_sad_u8 (n == nd - 1 ? v[d] & tail : v[d], brow[n], acc);
        }
      }
    }
  }
  acc += (uint32_t) __shfl_xor ((int) acc, 8);
  acc += (uint32_t) __shfl_xor ((int) acc, 16);
  acc += (uint32_t) __shfl_xor ((int) acc, 32);
  if (lane < 8)
    gstore < int32_t > (out + lane, ok ? (int32_t) acc : -1);
}

// The field of a pass as a source of the neighbour records of block (i, j), whose record is `rec`: single-reference and
// never intra, so every neighbour predicts.  A neighbour is addressed from `rec` -- a constant or one row away: the
// choice is one dependent chain per lane, and a record's address from the field's start would be three more 64-bit
// products on it.
struct SubpelRecords {
  const uint8_t *rec;
  int i, j, nbx;
  __device__ __forceinline__ bool operator () (int x, int y, int mode, int *vx, int *vy) const
  {
    mv_vector (rec + ((ptrdiff_t) (y - j) * nbx + (x - i)) * kMvBytes, mode - 1, vx, vy);
    return true;
  }
};

// block (i, j) of pass mvprec, by one lane: doubles the vector, predicts it, scores the centre and the candidates
__device__ __forceinline__ void
subpel_choose_block (const SubpelChain * ch, int i, int j)
{
  const int nbx = ch->nbx, ref = ch->ref;
  const size_t blk = (size_t) j * nbx + i;
  uint8_t *rec = mv_record (ch->field, nbx, i, j);
  int dx, dy, px, py;
  subpel_doubled (rec, ref, &dx, &dy);
  const SubpelRecords get = { rec, i, j, nbx };
  vector_prediction (get, i, j, ref + 1, &px, &py);     // schro_mf_vector_prediction (schromotion.c:259-312)

  const double lambda = ch->lambda;
  const uint32_t metric = gload < uint32_t > (rec + kMvMetric);
  int entropy = estimate_sint (dx - px) + estimate_sint (dy - py);
  double min_score = (double) entropy + lambda * (double) metric;       // (not contracted: the pragma above)
  int m = -1, min_error = 0;
  const int32_t *errors = ch->table + blk * 8;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int error = gload < int32_t > (errors + k);
    int ox, oy;
    subpel_offset (k, &ox, &oy);
    entropy = estimate_sint (dx + ox - px) + estimate_sint (dy + oy - py);
    const double score = (double) entropy + lambda * (double) error;
    if (error >= 0 && min_score > score) {
      min_score = score;
      min_error = error;
      m = k;
    }
  }
  int ndx = dx, ndy = dy;
  if (m >= 0) {
    int ox, oy;
    subpel_offset (m, &ox, &oy);
    ndx += ox;
    ndy += oy;
    gstore < uint32_t > (rec + kMvMetric, (uint32_t) min_error);
  }
  gstore < uint16_t > (rec + kMvDx + 2 * ref, (uint16_t) ndx);
  gstore < uint16_t > (rec + kMvDy + 2 * ref, (uint16_t) ndy);
}

__global__ __launch_bounds__ (kSubpelChooseThreads)
void subpel_choose_kernel (const SubpelChain * __restrict__ chains)
{
  const SubpelChain *ch = chains + blockIdx.x;
  // the blocks whose origin lies inside the picture: the others are skipped, their records stay as they are
  const int cols = min (ch->nbx, (ch->w + ch->xb - 1) / ch->xb), rws = min (ch->nby, (ch->h + ch->yb - 1) / ch->yb);
  walk_diagonals (cols, rws, (int) threadIdx.x, (int) blockDim.x, [&](int i, int j) {
        subpel_choose_block (ch, i, j);
      });
}

int
subpel_error_blocks ()
{
  return kSubpelWaves;
}

int
launch_subpel_error (hipStream_t stream, const SubpelChain * d_chains, int nchains, int total_groups, int mvprec)
{
  if (mvprec < 1 || mvprec > 3 || total_groups <= 0)
    return set_error (SCHRO_HIP_EINVAL, "sub-pel error launch: pass %d, %d workgroups", mvprec, total_groups);
  SCHRO_LAUNCH (subpel_error_kernel, dim3 (total_groups), dim3 (kSubpelThreads), 0, stream, d_chains, nchains, mvprec);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "sub-pel error launch: %s", hipGetErrorString (e));
  return 0;
}

int
launch_subpel_choose (hipStream_t stream, const SubpelChain * d_chains, int nchains, int mvprec)
{
  (void) mvprec;                // (the choice reads positions from no picture: the pass is in the tables)
  SCHRO_LAUNCH (subpel_choose_kernel, dim3 (nchains), dim3 (kSubpelChooseThreads), 0, stream, d_chains);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "sub-pel choice launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
