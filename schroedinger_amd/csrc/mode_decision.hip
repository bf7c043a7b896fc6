// mode_decision.hip -- schro_mode_decision entire (schromotionest.c:2587-2688): per superblock schro_do_split2, then
// schro_do_split1, schro_do_split0 if split 1 won, schro_do_split0_biref_zero with two references, the winner's records
// and the three statistics.  include/schro_hip.h restates the levels and lays the tables out; mode_common.h holds what is
// shared with the split-2 stage (mode_split2.hip), whose metric kernel fills the split-2 table here too, unchanged.
//
// The cut is DESIGN 4.13 / 4.14's.  mode_metric_kernel reads pictures for everything that depends on no decision: per
// superblock and reference 22 candidate vectors -- per quadrant its four sub-pel vectors and the level-1 vector, then the
// level-2 vector and the zero vector -- each with the bound test of split 1 on its own quadrant, the bound test of split 0
// on the superblock and its luma and chroma SAD over EACH of the four quadrants (a split-0 SAD is the sum: clipping and the
// bilinear form are per sample), and the bi-reference trial at zero vectors.  One WAVE per (superblock, reference,
// candidate), kModeUnits = 45 of them per superblock, kModeWaves per workgroup; a quadrant's component is cut into row
// segments of 16 samples, a lane takes segments lane, lane + 64, ..; the prediction of a segment is mode_split2.hip's.  A
// SAD the walk cannot ask for (neither bound test passed) is not read and written as -1.
//
// mode_choose_kernel, one workgroup per picture, walks the anti-diagonals of SUPERBLOCKS, one wave per superblock of the
// diagonal, a longer diagonal in rounds of kModeChooseWaves.  A superblock reads the final records of its left, upper and
// upper-left neighbours from `motion` (written before the barrier that ends their diagonal) and works on records of its own
// in LDS.  Within the wave: the split-2 level over its seven inner anti-diagonals, one lane per block (the per-block trial
// is the split-2 stage's, mode_common.h); then, with every lane computing the same values, the quadrants of split 1 in the
// C text's order, split 0 if split 1 won, the zero-vector trial, the choice and schro_block_fixup.  What depends on the
// decision and reads pictures -- the bi-reference metric of a split-1 quadrant and of split 0, both of the CHOSEN pair --
// is measured there by the wave's 64 lanes (mode_biref), with the reference's shared fetch buffers at mv_precision 2 and 3.
// The records the reference leaves in `motion` on the way (candidate trials, an invalid trial's leftovers) reach no result
// (tests/test_mode_ref.py shows it) and are not written; the trial stops at its first invalid quadrant.  After the last
// diagonal the workgroup counts the bad and the DC blocks and one lane sums mc_error in raster order of superblocks.
// No workgroup waits for another; every loop is bounded by the geometry; rows and columns of every image read are
// clamped (tap, motion_common.h), whatever a field holds.

#include "mode_common.h"

#pragma clang fp contract(off)

namespace schro {

constexpr int kModeWaves = 4;
constexpr int kModeThreads = kModeWaves * 64;
constexpr int kModeChooseWaves = 8;
constexpr int kModeChooseThreads = kModeChooseWaves * 64;
// the table entry of a superblock (include/schro_hip.h)
constexpr int kM_Cands = 22, kM_Level1 = 4, kM_Level2 = 20, kM_Zero = 21;
constexpr int kM_CandInts = 12, kM_Ok1 = 0, kM_Ok0 = 1, kM_Quad = 2;
constexpr int kM_RefInts = kM_Cands * kM_CandInts, kM_ZeroBi = 2 * kM_RefInts, kM_Ints = kM_ZeroBi + 4;
constexpr int kModeUnits = 2 * kM_Cands + 1;
constexpr int kTrialBytes = 24;         // SchroHipModeTrial

static_assert (kM_Ints == SCHRO_HIP_MODE_TABLE_INTS, "the table entry");
static_assert (sizeof (SchroHipModeTrial) == kTrialBytes, "the trial table");

// xmin > dx || ymin > dy || !(xmax > dx + width - 1) || !(ymax > dy + height - 1), negated: luma, the clipped block, the
// unscaled extension
__device__ __forceinline__ bool
mode_bound_ok (const Split2Job * jb, int X, int Y, int bw, int bh)
{
  return !(-jb->ext > X || -jb->ext > Y || !((jb->w << jb->prec) + jb->ext > X + bw - 1) || !((jb->h << jb->prec) + jb->ext > Y + bh - 1));
}

// a lane's share of the SAD of component k over the w x h samples at (x0, y0) against reference `ref` moved by the luma
// vector (vx, vy)
__device__ __forceinline__ uint32_t
mode_sad_share (const Split2Job * jb, int ref, int k, int x0, int y0, int w, int h, int vx, int vy, int lane)
{
  if (w <= 0 || h <= 0)
    return 0;
  const int c = k ? 1 : 0, pair = jb->pair, mvprec = jb->prec;
  const int tw = k ? jb->cw : jb->w, th = k ? jb->ch : jb->h;
  const int hs = k ? jb->hs : 0, vs = k ? jb->vs : 0;
  const int segs = (w + 15) >> 4;
  const uint8_t *plane = jb->src[k];
  const int stride = jb->src_stride[k];
  uint32_t acc = 0;
  for (int u = lane; u < segs * h; u += 64) {
    const int r = u / segs, seg = u - r * segs;
    const int tx = x0 + 16 * seg, ty = y0 + r, valid = w - 16 * seg;
    const u32x4 pred = predict (jb->up[ref][pair ? c : k], jb->up_stride[c], tw, th, (tx << mvprec) + (vx >> hs), (ty << mvprec) + (vy >> vs),
        mvprec, k ? pair : 0, k == 2);
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t m = split2_mask (valid, d);
      if (m)
        acc = __builtin_amdgcn_sad_u8 (pred[d] & m, scan_fetch4 (plane, stride, tw, th, tx + 4 * d, ty) & m, acc);
    }
  }
  return acc;
}

// The bi-reference trial over the `scale` x `scale` blocks that begin at block (x, y), by the whole wave: admissible, and
// then schro_metric_get_biref over luma and over U and V.  At mv_precision 2 and 3 the reference's fetch buffers are one
// per reference: luma is measured against V's prediction in its top-left corner and U against V's (mode_split2.hip).
__device__ __forceinline__ bool
mode_biref (const Split2Job * jb, int x, int y, int scale, int vx0, int vy0, int vx1, int vy1, uint32_t * luma, uint32_t * chroma, int lane)
{
  const int mvprec = jb->prec, pair = jb->pair;
  const int w0 = jb->w, h0 = jb->h, w1 = jb->cw, h1 = jb->ch;
  const int bx1 = jb->xb >> jb->hs, by1 = jb->yb >> jb->vs;
  const int xo0 = x * jb->xb, yo0 = y * jb->yb, xo1 = x * bx1, yo1 = y * by1;
  const int bw0 = min (scale * jb->xb, w0 - xo0), bh0 = min (scale * jb->yb, h0 - yo0);
  const int bw1 = max (min (scale * bx1, w1 - xo1), 0), bh1 = max (min (scale * by1, h1 - yo1), 0);
  *luma = 0, *chroma = 0;
  if (!mode_bound_ok (jb, (xo0 << mvprec) + vx0, (yo0 << mvprec) + vy0, bw0, bh0) || !mode_bound_ok (jb, (xo0 << mvprec) + vx1, (yo0 << mvprec) + vy1, bw0, bh0))
    return false;
  const bool shared = mvprec > 1;
  uint32_t bi_luma = 0, bi_chroma = 0;
  for (int k = 0; k < 3; k++) {
    const int c = k ? 1 : 0;
    const int tw = k ? w1 : w0, th = k ? h1 : h0, w = k ? bw1 : bw0, h = k ? bh1 : bh0;
    const int hs = k ? jb->hs : 0, vs = k ? jb->vs : 0;
    const int segs = (w + 15) >> 4;
    const uint8_t *plane = jb->src[k];
    const int stride = jb->src_stride[k], up_stride = jb->up_stride[c];
    for (int u = lane; u < segs * h; u += 64) {
      const int r = u / segs, seg = u - r * segs;
      const int tx = (k ? xo1 : xo0) + 16 * seg, ty = (k ? yo1 : yo0) + r, valid = w - 16 * seg;
      const bool corner = shared && k == 0 && r < bh1 && 16 * seg < bw1;        // V's prediction lies over this segment
      const bool from_v = corner || (shared && k == 1);
      u32x4 both = { 0, 0, 0, 0 };
      if (!(shared && k == 1)) {
        const u32x4 pred0 = predict (jb->up[0][pair ? c : k], up_stride, tw, th, (tx << mvprec) + (vx0 >> hs), (ty << mvprec) + (vy0 >> vs), mvprec,
            k ? pair : 0, k == 2);
        const u32x4 pred1 = predict (jb->up[1][pair ? c : k], up_stride, tw, th, (tx << mvprec) + (vx1 >> hs), (ty << mvprec) + (vy1 >> vs), mvprec,
            k ? pair : 0, k == 2);
        both = split2_average (pred0, pred1);
      }
      if (from_v) {
        const int xv = (xo1 + 16 * seg) << mvprec, yv = (yo1 + r) << mvprec;
        const u32x4 other0 = predict (jb->up[0][pair ? 1 : 2], jb->up_stride[1], w1, h1, xv + (vx0 >> jb->hs), yv + (vy0 >> jb->vs), mvprec, pair, 1);
        const u32x4 other1 = predict (jb->up[1][pair ? 1 : 2], jb->up_stride[1], w1, h1, xv + (vx1 >> jb->hs), yv + (vy1 >> jb->vs), mvprec, pair, 1);
        const u32x4 v = split2_average (other0, other1);
        const int nv = k ? 16 : bw1 - 16 * seg; // V's samples of this segment
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const uint32_t m = split2_mask (nv, d);
          both[d] = (v[d] & m) | (both[d] & ~m);
        }
      }
      uint32_t acc = 0;
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const uint32_t m = split2_mask (valid, d);
        if (m)
          acc = __builtin_amdgcn_sad_u8 (both[d] & m, scan_fetch4 (plane, stride, tw, th, tx + 4 * d, ty) & m, acc);
      }
      bi_chroma += k ? acc : 0;
      bi_luma += k ? 0 : acc;
    }
  }
  *luma = split2_wave_sum (bi_luma);
  *chroma = split2_wave_sum (bi_chroma);
  return true;
}

__global__ __launch_bounds__ (kModeThreads)
void mode_metric_kernel (const ModeJob * __restrict__ jobs, int njobs)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ModeJob *mj = jobs + find_job (jobs, njobs, (int) blockIdx.x);
  const Split2Job *jb = &mj->s;
  const int nbx = jb->nbx, sbx = nbx >> 2, nsb = sbx * (jb->nby >> 2);
  const int unit = ((int) blockIdx.x - mj->tile_base) * kModeWaves + wave;
  if (unit >= nsb * kModeUnits) // (wave-uniform; the kernel has no workgroup barrier)
    return;
  const int sbn = unit / kModeUnits, u = unit - sbn * kModeUnits;
  const int sy = sbn / sbx, i = 4 * (sbn - sy * sbx), j = 4 * sy;
  int32_t *t = mj->table + (size_t) sbn * kM_Ints;
  const int mvprec = jb->prec, nrefs = jb->num_refs;
  if (u == 2 * kM_Cands) {      // the bi-reference trial at zero vectors
    uint32_t luma = 0, chroma = 0;
    const bool ok = nrefs == 2 && mode_biref (jb, i, j, 4, 0, 0, 0, 0, &luma, &chroma, lane);
    if (lane < 4)
      gstore < int32_t > (t + kM_ZeroBi + lane, nrefs < 2 ? -1 : lane == 0 ? (int32_t) ok : lane == 1 ? (int32_t) luma : lane == 2 ? (int32_t) chroma : 0);
    return;
  }
  const int ref = u / kM_Cands, c = u - ref * kM_Cands;
  int32_t *out = t + ref * kM_RefInts + c * kM_CandInts;
  if (ref >= nrefs) {           // a reference the picture does not have
    if (lane < kM_CandInts)
      gstore < int32_t > (out + lane, -1);
    return;
  }
  // the candidate's vector
  const int q = c / 5, m = c - 5 * q;
  int vx = 0, vy = 0;
  if (c < kM_Level2) {
    const int x = i + 2 * (q & 1), y = j + 2 * (q >> 1);
    if (m < kM_Level1)
      mv_vector (mv_record (jb->field[ref], nbx, x + (m & 1), y + (m >> 1)), ref, &vx, &vy);
    else {
      mv_vector (mv_record (mj->hbm[ref][0], nbx, x, y), ref, &vx, &vy);
      vx = (int16_t) (vx * (1 << mvprec)), vy = (int16_t) (vy * (1 << mvprec));
    }
  } else if (c == kM_Level2) {
    mv_vector (mv_record (mj->hbm[ref][1], nbx, i, j), ref, &vx, &vy);
    vx = (int16_t) (vx * (1 << mvprec)), vy = (int16_t) (vy * (1 << mvprec));
  }
  const int w0 = jb->w, h0 = jb->h, w1 = jb->cw, h1 = jb->ch;
  const int bx0 = jb->xb, by0 = jb->yb, bx1 = jb->xb >> jb->hs, by1 = jb->yb >> jb->vs;
  const bool ok0 = mode_bound_ok (jb, vx + ((i * bx0) << mvprec), vy + ((j * by0) << mvprec), min (4 * bx0, w0 - i * bx0), min (4 * by0, h0 - j * by0));
  int ok1 = -1, luma[4], chroma[4];
#pragma unroll
  for (int qq = 0; qq < 4; qq++) {
    luma[qq] = -1, chroma[qq] = -1;
    const int x = i + 2 * (qq & 1), y = j + 2 * (qq >> 1);
    const int x0 = x * bx0, y0 = y * by0;
    if (x0 >= w0 || y0 >= h0)   // a quadrant outside the picture
      continue;
    bool need = ok0;
    if (c < kM_Level2 && q == qq) {
      ok1 = mode_bound_ok (jb, vx + (x0 << mvprec), vy + (y0 << mvprec), min (2 * bx0, w0 - x0), min (2 * by0, h0 - y0));
      need = need || ok1;
    }
    if (!need)
      continue;
    uint32_t a = mode_sad_share (jb, ref, 0, x0, y0, min (2 * bx0, w0 - x0), min (2 * by0, h0 - y0), vx, vy, lane);
    uint32_t b = mode_sad_share (jb, ref, 1, x * bx1, y * by1, min (2 * bx1, w1 - x * bx1), min (2 * by1, h1 - y * by1), vx, vy, lane);
    b += mode_sad_share (jb, ref, 2, x * bx1, y * by1, min (2 * bx1, w1 - x * bx1), min (2 * by1, h1 - y * by1), vx, vy, lane);
    luma[qq] = (int) split2_wave_sum (a);
    chroma[qq] = (int) split2_wave_sum (b);
  }
  if (lane < kM_CandInts) {
    int32_t v = 0;
    if (lane == kM_Ok1)
      v = ok1;
    else if (lane == kM_Ok0)
      v = ok0;
#pragma unroll
    for (int qq = 0; qq < 4; qq++) {
      if (lane == kM_Quad + 2 * qq)
        v = luma[qq];
      if (lane == kM_Quad + 2 * qq + 1)
        v = chroma[qq];
    }
    gstore < int32_t > (out + lane, v);
  }
}

// ---- the walk -------------------------------------------------------------------------------------------------------------

// a superblock's working state, one per wave
struct ModeWork {
  uint32_t w[16][3];            // the records its own blocks are seen as: flags, dx[0] | dx[1] << 16, dy[0] | dy[1] << 16
  uint32_t b[16][kMvDwords];    // block.mv: what the split-2 level decided
  int error[16], entropy[16];   // ... and its best_error, best_entropy per block
};

// neighbour records: of the wave's own superblock from LDS, everything else from the final field
struct ModeRecords {
  const uint8_t *motion;
  int nbx, sx, sy;
  const ModeWork *work;
  __device__ __forceinline__ void raw (int x, int y, uint32_t * flags, uint32_t * dx, uint32_t * dy) const
  {
    if ((x >> 2) == sx && (y >> 2) == sy) {
      const int n = (y & 3) * 4 + (x & 3);
      *flags = work->w[n][0], *dx = work->w[n][1], *dy = work->w[n][2];
    } else {
      const GlobalRecords field = { motion, nbx };
      field.raw (x, y, flags, dx, dy);
    }
  }
  __device__ __forceinline__ bool operator () (int x, int y, int mode, int *vx, int *vy) const
  {
    uint32_t flags, dx, dy;
    raw (x, y, &flags, &dx, &dy);
    return mv_predicts (flags, dx, dy, mode, vx, vy);
  }
};

// schro_motion_get_mode_prediction (schromotion.c:396-430)
__device__ __forceinline__ int
mode_mode_prediction (const ModeRecords & get, int x, int y)
{
  uint32_t a = 0, b = 0, c = 0, dx, dy;
  if (y == 0) {
    if (x == 0)
      return 0;
    get.raw (x - 1, 0, &a, &dx, &dy);
    return (int) (a & 3);
  }
  if (x == 0) {
    get.raw (0, y - 1, &a, &dx, &dy);
    return (int) (a & 3);
  }
  get.raw (x - 1, y, &a, &dx, &dy);
  get.raw (x, y - 1, &b, &dx, &dy);
  get.raw (x - 1, y - 1, &c, &dx, &dy);
  a &= 3, b &= 3, c &= 3;
  return (int) ((a & b) | (b & c) | (c & a));
}

// schro_motion_block_estimate_entropy for a record at its block's origin that predicts from the references in `modes`
__device__ __forceinline__ int
mode_entropy (const ModeRecords & get, int x, int y, const Split2Record & mv, int modes)
{
  if (mv.w[0] & 4)              // using_global travels with a hint's flags
    return 0;
  int entropy = 0;
#pragma unroll
  for (int mode = 1; mode <= 2; mode++)
    if (modes & mode) {
      int px, py;
      vector_prediction (get, x, y, mode, &px, &py);
      const int dx = (int16_t) (mv.w[3] >> (16 * (mode - 1))), dy = (int16_t) (mv.w[4] >> (16 * (mode - 1)));
      entropy += estimate_sint (dx - px) + estimate_sint (dy - py);
    }
  return entropy;
}

struct ModeHints {
  Split2Record rec[5];
  int slot[5];
  int n;
};

// One step of the hint lists of schro_get_best_mv_split1 / schro_get_best_split0_mv: skipped when its metric is INT_MAX
// or when (vector << compare) equals a listed vector (mv_already_in_list); stored with its vector << store.
__device__ __forceinline__ void
mode_hint_add (ModeHints & h, const Split2Record & rec, int slot, int ref, int compare, int store)
{
  if (rec.w[1] == (uint32_t) kSplit2IntMax)
    return;
  const int dx = (int16_t) (rec.w[3] >> (16 * ref)), dy = (int16_t) (rec.w[4] >> (16 * ref));
  bool listed = false;
#pragma unroll
  for (int k = 0; k < 5; k++)
    if (k < h.n) {
      const int hx = (int16_t) (h.rec[k].w[3] >> (16 * ref)), hy = (int16_t) (h.rec[k].w[4] >> (16 * ref));
      listed = listed || (dx * (1 << compare) == hx && dy * (1 << compare) == hy);
    }
  if (h.n && listed)
    return;
  Split2Record r = rec;
  if (store) {
    const uint32_t keep = ~(0xffffu << (16 * ref));
    r.w[3] = (r.w[3] & keep) | (((uint32_t) (dx * (1 << store)) & 0xffffu) << (16 * ref));
    r.w[4] = (r.w[4] & keep) | (((uint32_t) (dy * (1 << store)) & 0xffffu) << (16 * ref));
  }
#pragma unroll
  for (int k = 0; k < 5; k++)
    if (k == h.n) {
      h.rec[k] = r;
      h.slot[k] = slot;
    }
  h.n++;
}

struct ModeBest {
  bool valid;
  Split2Record mv;
  int error, entropy, slot;
};

// The candidate loop of schro_get_best_mv_split1 (split 1, quadrant q at block (x, y)) and of schro_get_best_split0_mv
// (split 0): the bound test and the SADs come from the table.
__device__ __forceinline__ ModeBest
mode_best_hint (const ModeHints & h, const int32_t * entries, const ModeRecords & get, int x, int y, int ref, int split, int q, double lambda)
{
  ModeBest best;
  best.valid = false, best.error = 0, best.entropy = 0, best.slot = 0;
  best.mv = h.rec[0];
  double min_score = __builtin_huge_val ();
  int best_luma = 0, best_chroma = 0;
#pragma unroll
  for (int m = 0; m < 5; m++) {
    if (m >= h.n)
      continue;
    const int32_t *e = entries + h.slot[m] * kM_CandInts;
    if (gload < int32_t > (e + (split ? kM_Ok1 : kM_Ok0)) != 1)
      continue;
    int luma = 0, chroma = 0;
    if (split)
      luma = gload < int32_t > (e + kM_Quad + 2 * q), chroma = gload < int32_t > (e + kM_Quad + 2 * q + 1);
    else {
#pragma unroll
      for (int qq = 0; qq < 4; qq++) {
        const int a = gload < int32_t > (e + kM_Quad + 2 * qq), b = gload < int32_t > (e + kM_Quad + 2 * qq + 1);
        luma += a == -1 ? 0 : a, chroma += a == -1 ? 0 : b;
      }
    }
    Split2Record mv = h.rec[m];
    mv.w[0] = (mv.w[0] & ~0x1bu) | ((uint32_t) split << 3) | (uint32_t) (ref + 1);    // split, pred_mode; using_global stays
    const int entropy = mode_entropy (get, x, y, mv, ref + 1);
    const double score = (double) entropy + (double) (luma + chroma) * lambda;
    if (min_score > score) {
      min_score = score;
      best.valid = true;
      best.mv = mv;
      best.entropy = entropy;
      best.slot = h.slot[m];
      best_luma = luma, best_chroma = chroma;
    }
  }
  if (best.valid) {
    best.error = best_luma + best_chroma;
    best.mv.w[1] = (uint32_t) (best_luma >> (split ? 2 : 4));
    best.mv.w[2] = (uint32_t) (best_chroma >> (split ? 2 : 4));
  }
  return best;
}

struct ModeTrial {
  int state, error, entropy;
  double score;
};

__device__ __forceinline__ void
mode_store_trial (uint8_t * p, const ModeTrial & t)
{
  const bool ok = t.state == 1;
  gstore < int32_t > ((int32_t *) p, t.state);
  gstore < int32_t > ((int32_t *) p + 1, ok ? t.error : 0);
  gstore < int32_t > ((int32_t *) p + 2, ok ? t.entropy : 0);
  gstore < int32_t > ((int32_t *) p + 3, 0);
  gstore < double >((double *) (p + 16), ok ? t.score : 0.0);
}

// Everything of a superblock behind its split-2 level, with every lane of the wave computing the same values.
__device__ __forceinline__ void
mode_superblock (const ModeJob * mj, ModeWork * work, int sx, int sy, int lane)
{
  const Split2Job *jb = &mj->s;
  const int nbx = jb->nbx, nrefs = jb->num_refs, mvprec = jb->prec;
  const int i = 4 * sx, j = 4 * sy, sbn = sy * (nbx >> 2) + sx;
  const double lambda = jb->lambda;
  const int32_t *table = mj->table + (size_t) sbn * kM_Ints;
  const ModeRecords get = { jb->motion, nbx, sx, sy, work };

  // schro_do_split2's sums
  ModeTrial trial[4];
  {
    uint32_t error = 0, entropy = 0;
    for (int n = 0; n < 16; n++)
      error += (uint32_t) work->error[n], entropy += (uint32_t) work->entropy[n];
    trial[0].state = 1, trial[0].error = (int) error, trial[0].entropy = (int) entropy;
    trial[0].score = (double) (int) entropy + lambda * (double) (int) error;
  }
  trial[1].state = 0, trial[2].state = -1, trial[3].state = -1;
  double min_score = trial[0].score;
  int winner = 0;               // the index of the winning trial

  // schro_do_split1: the quadrants in the C text's order
  Split2Record quad[4], mf[2][4];
  int mf_slot[2][4];
  bool valid1 = true;
  uint32_t total_error = 0, total_entropy = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    quad[q] = { {0, 0, 0, 0, 0} };
    mf[0][q] = mf[1][q] = { {0, (uint32_t) kSplit2IntMax, 0, 0, 0} };
    mf_slot[0][q] = mf_slot[1][q] = 0;
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    if (!valid1)                // (the reference goes on; what it writes then reaches nothing)
      continue;
    const int ii = 2 * (q & 1), jj = 2 * (q >> 1), x = i + ii, y = j + jj;
    Split2Record best = { {0x09u, (uint32_t) kSplit2IntMax, (uint32_t) kSplit2IntMax, 0, 0} };
    bool have = false;
    if (!(jb->w > x * jb->xb) || !(jb->h > y * jb->yb)) {
      // outside the picture: the predicted form
      int mode = mode_mode_prediction (get, x, y);
      if (mode != 1 && mode != 2)
        mode = 1;
      int px, py;
      vector_prediction (get, x, y, 1, &px, &py);
      best = { {0x08u | (uint32_t) mode, 0, 0, ((uint32_t) px & 0xffffu) << (16 * (mode - 1)), ((uint32_t) py & 0xffffu) << (16 * (mode - 1))} };
      total_entropy += 2;
      mf[0][q] = { {0x09u, 0, 0, 0, 0} };
      mf[1][q] = { {0x0au, 0, 0, 0, 0} };
      mf_slot[0][q] = mf_slot[1][q] = kM_Zero;
      have = true;
    } else {
      double quad_score = __builtin_huge_val ();
      int best_entropy = kSplit2IntMax, best_error = kSplit2IntMax, best_chroma = kSplit2IntMax;
      ModeBest one[2];
#pragma unroll
      for (int ref = 0; ref < 2; ref++) {
        one[ref].valid = false;
        if (ref >= nrefs)
          continue;
        ModeHints h;
        h.n = 0;
#pragma unroll
        for (int m = 0; m < 4; m++)
          mode_hint_add (h, split2_load (mv_record (jb->field[ref], nbx, x + (m & 1), y + (m >> 1))), 5 * q + m, ref, mvprec, 0);
        mode_hint_add (h, split2_load (mv_record (mj->hbm[ref][0], nbx, x, y)), 5 * q + kM_Level1, ref, mvprec, mvprec);
        one[ref] = mode_best_hint (h, table + ref * kM_RefInts, get, x, y, ref, 1, q, lambda);
        if (one[ref].valid) {
          mf[ref][q] = one[ref].mv;
          mf_slot[ref][q] = one[ref].slot;
          const double score = (double) one[ref].entropy + lambda * (double) one[ref].error;
          if (quad_score > score) {
            quad_score = score;
            best = one[ref].mv;
            best_entropy = one[ref].entropy;
            best_error = one[ref].error;
            have = true;
          }
        }
      }
      if (nrefs > 1 && one[0].valid && one[1].valid) {
        Split2Record both = one[0].mv;
        both.w[3] = (both.w[3] & 0xffffu) | (one[1].mv.w[3] & 0xffff0000u);
        both.w[4] = (both.w[4] & 0xffffu) | (one[1].mv.w[4] & 0xffff0000u);
        both.w[0] |= 3u;
        uint32_t luma, chroma;
        if (mode_biref (jb, x, y, 2, (int16_t) both.w[3], (int16_t) both.w[4], (int16_t) (both.w[3] >> 16), (int16_t) (both.w[4] >> 16), &luma, &chroma, lane)) {
          const double score = (double) (one[0].entropy + one[1].entropy) + lambda * (double) (int) (luma + chroma);
          both.w[1] = luma >> 2;
          both.w[2] = chroma >> 2;
          if (quad_score > score) {
            best_error = (int) luma;
            best_chroma = (int) chroma;
            best_entropy = one[0].entropy + one[1].entropy;
            best = both;
            quad_score = score;
          }
        }
      }
      if (have) {
        total_error += (uint32_t) best_error + (uint32_t) best_chroma;        // best_chroma stays INT_MAX unless the pair won
        total_entropy += (uint32_t) best_entropy;
      }
    }
    if (!have) {
      valid1 = false;
      continue;
    }
    quad[q] = best;
    // *mv = best_mv; set_split1_motion
#pragma unroll
    for (int n = 0; n < 4; n++) {
      const int at = (jj + (n >> 1)) * 4 + ii + (n & 1);
      work->w[at][0] = best.w[0], work->w[at][1] = best.w[3], work->w[at][2] = best.w[4];
    }
  }
  if (valid1) {
    trial[1].state = 1, trial[1].error = (int) total_error, trial[1].entropy = (int) total_entropy;
    trial[1].score = (double) (int) total_entropy + lambda * (double) (int) total_error;
  }
  // tryblock.mv[0][0] through the later trials
  Split2Record first = quad[0], zero_rec = first, split0_rec = first;
  if (valid1 && min_score > trial[1].score) {
    winner = 1;
    min_score = trial[1].score;
    // schro_do_split0
    trial[2].state = 0;
    double level_score = __builtin_huge_val ();
    Split2Record best = first;
    int best_error = kSplit2IntMax, best_entropy = kSplit2IntMax;
    bool have = false;
    ModeBest one[2];
#pragma unroll
    for (int ref = 0; ref < 2; ref++) {
      one[ref].valid = false;
      if (ref >= nrefs)
        continue;
      ModeHints h;
      h.n = 0;
#pragma unroll
      for (int q = 0; q < 4; q++)
        mode_hint_add (h, mf[ref][q], mf_slot[ref][q], ref, 0, 0);        // (the slot of the quadrant's winner in the table)
      mode_hint_add (h, split2_load (mv_record (mj->hbm[ref][1], nbx, i, j)), kM_Level2, ref, mvprec, mvprec);
      one[ref] = mode_best_hint (h, table + ref * kM_RefInts, get, i, j, ref, 0, 0, lambda);
      if (one[ref].valid) {
        const double score = (double) one[ref].entropy + lambda * (double) one[ref].error;
        if (level_score > score) {
          level_score = score;
          best = one[ref].mv;
          best_entropy = one[ref].entropy;
          best_error = one[ref].error;
          have = true;
        }
      }
    }
    if (nrefs > 1 && one[0].valid && one[1].valid) {
      Split2Record both = { {3u, (uint32_t) kSplit2IntMax, 0, (one[0].mv.w[3] & 0xffffu) | (one[1].mv.w[3] & 0xffff0000u),
              (one[0].mv.w[4] & 0xffffu) | (one[1].mv.w[4] & 0xffff0000u)} };
      const int entropy = mode_entropy (get, i, j, both, 3);
      uint32_t luma, chroma;
      if (mode_biref (jb, i, j, 4, (int16_t) both.w[3], (int16_t) both.w[4], (int16_t) (both.w[3] >> 16), (int16_t) (both.w[4] >> 16), &luma, &chroma, lane)) {
        both.w[1] = luma >> 4;
        both.w[2] = chroma >> 4;
        const int error = (int) (luma + chroma);
        const double score = (double) entropy + lambda * (double) error;
        if (level_score > score) {
          level_score = score;
          best = both;
          best_error = error;
          best_entropy = entropy;
          have = true;
        }
      }
    }
    if (have) {
      trial[2].state = 1, trial[2].error = best_error, trial[2].entropy = best_entropy;
      trial[2].score = (double) best_entropy + lambda * (double) best_error;
      first = best;             // block->mv[0][0] = best_mv
      if (min_score > trial[2].score) {
        winner = 2;             // (min_score stays split 1's: the zero-vector trial is compared with that)
        split0_rec = best;
      }
    }
  }
  if (nrefs > 1) {
    // schro_do_split0_biref_zero over tryblock.mv[0][0] as the earlier trials left it
    trial[3].state = 0;
    zero_rec = first;
    zero_rec.w[0] = (zero_rec.w[0] & ~0x1fu) | 3u;
    zero_rec.w[3] = 0, zero_rec.w[4] = 0;
    const int entropy = mode_entropy (get, i, j, zero_rec, 3);
    if (gload < int32_t > (table + kM_ZeroBi) == 1) {
      const int luma = gload < int32_t > (table + kM_ZeroBi + 1), chroma = gload < int32_t > (table + kM_ZeroBi + 2);
      zero_rec.w[1] = (uint32_t) (luma >> 4);
      zero_rec.w[2] = (uint32_t) (chroma >> 4);
      trial[3].state = 1, trial[3].error = luma + chroma, trial[3].entropy = entropy;
      trial[3].score = (double) entropy + lambda * (double) (luma + chroma);
      if (min_score > trial[3].score)
        winner = 3;
    }
  }
  // the winner's records (schro_block_fixup, schro_motion_copy_to), its sums and the trials
  if (lane < 16) {
    const int ii = lane & 3, jj = lane >> 2;
    Split2Record rec;
    if (winner == 0) {
#pragma unroll
      for (int n = 0; n < kMvDwords; n++)
        rec.w[n] = work->b[lane][n];
    } else if (winner == 1) {
      const int q = (ii >> 1) + 2 * (jj >> 1);
      rec = quad[0];
#pragma unroll
      for (int k = 1; k < 4; k++)
        if (q == k)
          rec = quad[k];
    } else
      rec = winner == 2 ? split0_rec : zero_rec;
    split2_store (mv_record (jb->motion, nbx, i + ii, j + jj), rec);
  }
  if (lane == 0) {
    ModeTrial won = trial[0];
#pragma unroll
    for (int k = 1; k < 4; k++)
      if (winner == k)
        won = trial[k];
    uint8_t *sb = jb->sb + (size_t) sbn * 16;
    gstore < int32_t > ((int32_t *) sb, won.error);
    gstore < int32_t > ((int32_t *) sb + 1, won.entropy);
    gstore < double >((double *) (sb + 8), won.score);
#pragma unroll
    for (int k = 0; k < 4; k++)
      mode_store_trial (mj->trials + ((size_t) sbn * 4 + k) * kTrialBytes, trial[k]);
  }
}

__global__ __launch_bounds__ (kModeChooseThreads)
void mode_choose_kernel (const ModeJob * __restrict__ jobs)
{
  __shared__ ModeWork works[kModeChooseWaves];
  __shared__ int bad_blocks, dc_blocks;
  const ModeJob *mj = jobs + blockIdx.x;
  const Split2Job *jb = &mj->s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nbx = jb->nbx, nby = jb->nby, sbx = nbx >> 2, sby = nby >> 2, nsb = sbx * sby;
  ModeWork *work = works + wave;
  for (int d = 0; d < sbx + sby - 1; d++) {
    const int lo = max (0, d - (sbx - 1)), hi = min (d, sby - 1);
    for (int base = lo; base <= hi; base += kModeChooseWaves) {
      const int sy = base + wave, sx = d - sy;
      const bool active = sy <= hi;
      // the split-2 level over the superblock's inner anti-diagonals, one lane per block
      const int ii = lane & 3, jj = (lane >> 2) & 3, x = 4 * sx + ii, y = 4 * sy + jj;
      for (int inner = 0; inner < 7; inner++) {
        if (active && lane < 16 && ii + jj == inner) {
          Split2Record rec = { {0x11u, 0, 0, 0, 0} };      // outside the picture: the constant best_mv, total_entropy += 2
          int error = 0, entropy = 2;
          if (x * jb->xb < jb->w && y * jb->yb < jb->h) {
            const ModeRecords get = { jb->motion, nbx, sx, sy, work };
            rec = split2_block_trial (jb, get, x, y, &error, &entropy);
          }
#pragma unroll
          for (int n = 0; n < kMvDwords; n++)
            work->b[lane][n] = rec.w[n];
          work->w[lane][0] = rec.w[0], work->w[lane][1] = rec.w[3], work->w[lane][2] = rec.w[4];
          work->error[lane] = error, work->entropy[lane] = entropy;
        }
        __syncthreads ();       // (every wave of the workgroup passes here seven times per round)
      }
      if (active)
        mode_superblock (mj, work, sx, sy, lane);
    }
    __threadfence ();
    __syncthreads ();           // the next diagonal reads this one's records
  }
  // the statistics (schromotionest.c:2655-2681)
  if (threadIdx.x == 0)
    bad_blocks = 0, dc_blocks = 0;
  __syncthreads ();
  const int block_size = 16 * jb->xb * jb->yb * 2 / 3;
  int bad = 0, dc = 0;
  for (int n = (int) threadIdx.x; n < nbx * nby; n += (int) blockDim.x)
    dc += (gload < uint32_t > (jb->motion + (size_t) n * kMvBytes + kMvFlags) & 3u) == 0;
  for (int s = (int) threadIdx.x; s < nsb; s += (int) blockDim.x)
    bad += gload < int32_t > ((const int32_t *) (jb->sb + (size_t) s * 16)) > 10 * block_size;
  if (dc)
    atomicAdd (&dc_blocks, dc);
  if (bad)
    atomicAdd (&bad_blocks, bad);
  __syncthreads ();
  if (threadIdx.x == 0) {
    double total = 0.0;         // in raster order of superblocks
    for (int s = 0; s < nsb; s++) {
      const int error = gload < int32_t > ((const int32_t *) (jb->sb + (size_t) s * 16));
      total += (double) error * error / (double) (block_size * block_size);
    }
    gstore < double >(mj->stats, total / (240.0 * 240.0) / nbx * nby / 16);
    gstore < double >(mj->stats + 1, ((double) bad_blocks) / (nbx * nby / 16));
    gstore < double >(mj->stats + 2, ((double) dc_blocks) / (nbx * nby));
  }
}

int
mode_metric_units ()
{
  return kModeUnits;
}

int
mode_metric_waves ()
{
  return kModeWaves;
}

int
launch_mode_metric (hipStream_t stream, const ModeJob * d_jobs, int njobs, int total_groups)
{
  if (njobs <= 0 || total_groups <= 0)
    return set_error (SCHRO_HIP_EINVAL, "mode metric launch: %d pictures, %d workgroups", njobs, total_groups);
  SCHRO_LAUNCH (mode_metric_kernel, dim3 (total_groups), dim3 (kModeThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "mode metric launch: %s", hipGetErrorString (e));
  return 0;
}

int
launch_mode_choose (hipStream_t stream, const ModeJob * d_jobs, int njobs)
{
  if (njobs <= 0)
    return set_error (SCHRO_HIP_EINVAL, "mode choice launch: %d pictures", njobs);
  SCHRO_LAUNCH (mode_choose_kernel, dim3 (njobs), dim3 (kModeChooseThreads), 0, stream, d_jobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "mode choice launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
