// rough_hint.hip -- the hierarchical rough motion search (schro_rough_me_heirarchical_scan, schroroughmotion.c:47-300):
// the nohint level and the hint levels below it, one launch per call.  Integer arithmetic only: bit-exact.
//
// One workgroup per (picture, reference) chain, SCHRO_HIP_ROUGH_WAVES waves at the most.  The chain's levels run one after
// the other inside the launch, coarse to fine.  A block of a hint level reads three records of its own level (left, above,
// above-left) and up to four of the level above, so raster order relaxes to anti-diagonals d = (i + j) / skip: the waves
// take the blocks of a diagonal in turn, __syncthreads () separates diagonals and levels.  The fields live in global
// memory: one workgroup is one CU and one L1, so what a wave stored in front of the barrier the others read behind it.
// No wave waits on anything another workgroup writes; every loop is bounded by the geometry.
//
// Per block the wave
//   * stages the block in its share of the LDS (scan_common.h) -- once, for the candidates and the scan;
//   * tests the candidates (schroroughmotion.c:232-268): lane = candidate + 8 * row group, candidates in the reference's
//     order (zero vector, parents m = 0 .. 3, left, above, above-left), each lane the SAD of its rows against the
//     reference picture in global memory (a candidate that is not skipped lies inside the picture), summed over the row
//     groups, then the minimum of (metric << 3) | candidate: strictly smaller wins, the first of equals wins; if every
//     candidate is skipped the zero vector stays;
//   * sets up the window around the winner >> shift (schro_metric_scan_setup), stages it and runs the scan of
//     metric_scan_kernel (81 positions at distance 4: two passes of the 64 lanes);
//   * stores metric and dx[ref], dy[ref] << shift as int16.
// A block of no width or height (x_num_blocks * xbsep beyond the picture) has every candidate skipped and SAD 0 at every
// position: the gravity vector is kept with metric 0 -- also where the reference's gravity position lies outside the
// window, which happens for such blocks only.  A window of no width or height stores 0, 0, INT_MAX.
// The launch first writes every record of every field as schro_motion_field_set (mf, 0, 1) leaves it.
// That preamble, the walk over the anti-diagonals, the scan with its three stores and the launch are motion_common.h's
// (fill_fields, walk_diagonals, scan_and_store, launch_chains), shared with hier_bm.hip; the ScanRules below say where
// this search differs.

#include "motion_common.h"

namespace schro {

// block (i, j) of level lv, by one wave
__device__ __forceinline__ void
rough_block (const RoughChain * ch, const RoughLevel & lv, int i, int j, uint32_t * lds, int lane)
{
  const int nbx = ch->nbx, nby = ch->nby, xb = ch->xb, yb = ch->yb, ref = ch->ref;
  const int shift = lv.shift, skip = 1 << shift, w = lv.w, h = lv.h;
  const int x = (i >> shift) * xb, y = (j >> shift) * yb;       // == i * xb >> shift: i is a multiple of skip
  const int bw = min (w - x, xb), bh = min (h - y, yb);
  const bool empty = bw <= 0 || bh <= 0;
  const int nd = empty ? 0 : scan_block_pitch (bw) >> 2;
  const int rows = empty ? 0 : bh;
  const uint32_t tail = scan_tail_mask (bw);
  uint32_t *block = lds, *window = lds + nd * rows;

  wave_sync ();                 // (the block before this one is through with the LDS)
  scan_stage_block (block, lv.frame, lv.frame_stride, w, h, x, y, nd, rows, tail, lane);
  wave_sync ();

  int gx = 0, gy = 0;           // the scan's vector: the winner >> shift
  if (lv.hint) {
    const int c = lane & 7;
    const int mask = ~((1 << (shift + 1)) - 1);
    const uint8_t *rec = nullptr;
    if (c >= 1 && c <= 4) {
      const int m = c - 1;
      const int l = (i + skip * (-1 + 2 * (m & 1))) & mask, k = (j + skip * (-1 + (m & 2))) & mask;    // negative stays negative
      if (l >= 0 && l < nbx && k >= 0 && k < nby)
        rec = mv_record (lv.hint, nbx, l, k);
    } else if (c >= 5) {
      rec = mv_neighbour (lv.field, nbx, i, j, skip, c - 5);
    }
    int cdx = 0, cdy = 0;
    if (rec)
      mv_vector (rec, ref, &cdx, &cdy);
    const int cx = (i * xb + cdx) >> shift, cy = (j * yb + cdy) >> shift;
    // :245-260: skipped in front of the picture, with an empty block, or where the reference picture ends inside the block
    const bool ok = (c == 0 || rec) && !empty && cx >= 0 && cy >= 0 && max (0, w - cx) >= bw && max (0, h - cy) >= bh;
    uint32_t acc = 0;
    if (ok)
      for (int r = lane >> 3; r < rows; r += 8) {
        const uint32_t *brow = block + r * nd;
        for (int d = 0; d < nd; d++) {
          uint32_t v = scan_fetch4 (lv.ref, lv.ref_stride, w, h, cx + 4 * d, cy + r);
          if (d == nd - 1)
            v &= tail;
          acc = __builtin_amdgcn_sad_u8 (v, brow[d], acc);
        }
      }
    for (int off = 8; off < 64; off <<= 1)
      acc += (uint32_t) __shfl_xor ((int) acc, off);
    uint32_t key = ok ? (acc << 3) | (uint32_t) c : 0xffffffffu;
    for (int off = 1; off < 8; off <<= 1)
      key = min (key, (uint32_t) __shfl_xor ((int) key, off));
    const int win = key == 0xffffffffu ? 0 : (int) (key & 7u);  // lane `win` holds candidate `win`
    gx = __shfl (cdx, win) >> shift;
    gy = __shfl (cdy, win) >> shift;
  }

  // (:106-109: the gravity of the nohint level is the window's first position; a window of no width or height stores 0, 0)
  const ScanRules rules = { !lv.hint, true, false, empty };
  scan_and_store (lv, lv.ref, lv.ref_stride, w, h, shift, mv_record (lv.field, nbx, i, j), ref, x, y, bw, bh, gx, gy, block, window, rules, lane);
}

__global__ __launch_bounds__ (kChainThreads)
void rough_hint_kernel (const RoughChain * __restrict__ chains, int lds_per_wave)
{
  extern __shared__ __attribute__ ((aligned (16))) uint32_t rough_lds[];
  const RoughChain *ch = chains + blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  uint32_t *lds = rough_lds + (size_t) wave * (lds_per_wave >> 2);
  const int nbx = ch->nbx, nby = ch->nby, nlevels = ch->nlevels;

  fill_fields (ch, [](const RoughLevel &) { return 1u; });     // schro_motion_field_set (mf, 0, 1)

  for (int n = 0; n < nlevels; n++) {
    const RoughLevel lv = ch->level[n];
    const int shift = lv.shift;
    const int cols = (nbx + (1 << shift) - 1) >> shift, rws = (nby + (1 << shift) - 1) >> shift;       // the level's grid
    if (!lv.hint) {
      // every block on its own
      for (int t = wave; t < cols * rws; t += nwaves) {
        const int bj = t / cols;
        rough_block (ch, lv, (t - bj * cols) << shift, bj << shift, lds, lane);
      }
      __syncthreads ();
      continue;
    }
    walk_diagonals (cols, rws, wave, nwaves, [&](int bi, int bj) {
          rough_block (ch, lv, bi << shift, bj << shift, lds, lane);
        });
  }
}

int
launch_rough_hint (hipStream_t stream, const RoughChain * d_chains, int nchains, size_t lds_per_wave)
{
  return launch_chains (rough_hint_kernel, "rough search", stream, d_chains, nchains, lds_per_wave);
}

}                               // namespace schro
