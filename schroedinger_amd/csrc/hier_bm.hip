// hier_bm.hip -- hierarchical block matching, the DEFAULT encoder's motion search (schro_hbm_scan and
// schro_hierarchical_bm_scan_hint, schrohierbm.c:158-383): the levels of a chain, level 0 among them, one launch per call.
// Integer arithmetic only: bit-exact.
//
// One workgroup per (picture, reference) chain, SCHRO_HIP_ROUGH_WAVES waves at the most, as rough_hint.hip: the chain's
// levels run one after the other inside the launch, coarse to fine.  EVERY level's blocks read three records of their own
// level (left, above, above-left) -- the top level too, which has no parents -- so every level is a walk over the
// anti-diagonals d = (i + j) / skip: the waves take the blocks of a diagonal in turn, __syncthreads () separates diagonals
// and levels.  The fields live in global memory: one workgroup is one CU and one L1, so what a wave stored in front of the
// barrier the others read behind it.  No wave waits on anything another workgroup writes; every loop is bounded by the
// geometry.
//
// Per block whose origin lies inside the level's luma plane (:244-247; the others keep the field-set record) the wave
//   * stages the clipped luma block in its share of the LDS (scan_common.h) -- once, for the candidates and the scan;
//   * gathers the candidates (:258-294), lane c = candidate c of the FULL list (zero vector, the five parents of the star,
//     left, above, above-left: nine slots, absent ones marked) and drops every entry that a later present entry equals in
//     dx[ref], dy[ref] (:298-321: the survivors stand in order of LAST occurrence; slot order is list order);
//   * tests the survivors (:326-346): lane = slot + 16 * row group, the vector >> shift clamped as the reference clamps
//     it, each lane the SAD of its rows of the luma block (LDS) and of both chroma blocks (schro_metric_block_sad_slow:
//     chroma at x >> h_shift, clipped to the frame's plane) against the reference frame in global memory, coordinates
//     clamped to the plane (the edge-extended apron); summed over the row groups, then the minimum of (metric << 4) |
//     slot: strictly smaller wins, the first of equals wins;
//   * sets up the window of h_range around the winner >> shift clamped as :357-358 (schro_metric_scan_setup), stages it
//     and runs the scan of metric_scan_kernel with the start vector as gravity, luma only;
//   * stores metric and dx[ref], dy[ref] << shift as int16 (flags, chroma_metric 0 and the other reference's 0 are the
//     field-set record's already).
// The host refuses an extension under max (xbsep, ybsep): with it schro_frame_block_is_valid holds for every candidate
// (the clamp keeps x + dx in -width0 .. width), the window has a position and contains the start vector.  The launch first
// writes every record of every field as schro_motion_field_set (mf, split, ref + 1) leaves it.
// That preamble, the walk, the scan with its three stores and the launch are motion_common.h's (fill_fields,
// walk_diagonals, scan_and_store, launch_chains), shared with rough_hint.hip; the ScanRules below say where this search
// differs.

#include "motion_common.h"

namespace schro {

constexpr int kHbmSlots = 9;    // LIST_LENGTH, schrohierbm.c:191

__device__ __forceinline__ int
hbm_clamp (int x, int a, int b)
{
  return x < a ? a : (x > b ? b : x);   // CLAMP, schroutils.h
}

// the SAD of rows r0, r0 + 4, .. of a chroma block: cw x chh samples of `frame` from (fx, fy) -- inside the plane --
// against `ref` from (rx, ry), coordinates clamped to the pw x ph plane
__device__ __forceinline__ uint32_t
hbm_chroma_sad (const uint8_t * frame, int frame_stride, const uint8_t * ref, int ref_stride, int pw, int ph, int fx, int fy, int rx, int ry,
    int cw, int chh, int r0, uint32_t acc)
{
  if (cw <= 0)
    return acc;
  const int nd = (cw + 3) >> 2;
  const uint32_t tail = scan_tail_mask (cw);
  for (int r = r0; r < chh; r += 4)
    for (int d = 0; d < nd; d++) {
      uint32_t a = scan_fetch4 (frame, frame_stride, pw, ph, fx + 4 * d, fy + r);
      uint32_t b = scan_fetch4 (ref, ref_stride, pw, ph, rx + 4 * d, ry + r);
      if (d == nd - 1) {
        a &= tail;
        b &= tail;
      }
      acc = __builtin_amdgcn_sad_u8 (a, b, acc);
    }
  return acc;
}

// block (i, j) of level lv, by one wave
__device__ __forceinline__ void
hbm_block (const HbmChain * ch, const HbmLevel & lv, int i, int j, uint32_t * lds, int lane)
{
  const int nbx = ch->nbx, nby = ch->nby, xb = ch->xb, yb = ch->yb, ref = ch->ref;
  const int shift = lv.shift, skip = 1 << shift, w = lv.w, h = lv.h;
  const int x = (i >> shift) * xb, y = (j >> shift) * yb;       // == i * xb >> shift: i is a multiple of skip
  if (!(w > x) || !(h > y))     // :244-247 (wave-uniform)
    return;
  const int bw = min (w - x, xb), bh = min (h - y, yb);         // > 0
  const int nd = scan_block_pitch (bw) >> 2;
  const uint32_t tail = scan_tail_mask (bw);
  uint32_t *block = lds, *window = lds + nd * bh;

  wave_sync ();                 // (the block before this one is through with the LDS)
  scan_stage_block (block, lv.frame[0], lv.frame_stride[0], w, h, x, y, nd, bh, tail, lane);
  wave_sync ();

  // ---- the candidates: slot c of the list in lane c (and in lanes c + 16, c + 32, c + 48) ----
  const int c = lane & 15, rg = lane >> 4;
  const uint8_t *rec = nullptr;
  if (c >= 1 && c <= 5) {
    if (lv.hint) {
      const int m = c - 1;
      const int mask = ~((1 << (shift + 1)) - 1);
      const int ox = m == 1 ? -1 : (m == 2 ? 1 : 0), oy = m == 3 ? -1 : (m == 4 ? 1 : 0);      // :266
      const int ll = (i & mask) + ox * skip * 2, kk = (j & mask) + oy * skip * 2;
      if (ll >= 0 && ll < nbx && kk >= 0 && kk < nby)
        rec = mv_record (lv.hint, nbx, ll, kk);
    }
  } else if (c >= 6 && c <= 8) {
    rec = mv_neighbour (lv.field, nbx, i, j, skip, c - 6);
  }
  int cdx = 0, cdy = 0;
  if (rec)
    mv_vector (rec, ref, &cdx, &cdy);
  const bool present = c == 0 || rec != nullptr;
  // :298-321: gone when a later present entry holds the same vector (every lane of a 16-lane row holds the same list)
  bool alive = present;
  const int vec = (cdx & 0xffff) | (cdy << 16);
  for (int s = 1; s < kHbmSlots; s++) {
    const int ovec = __shfl (vec, (lane & 48) + s);
    const int opresent = __shfl ((int) present, (lane & 48) + s);
    if (s > c && opresent && ovec == vec)
      alive = false;
  }

  // ---- the choice: the SAD over the three components at the clamped vector ----
  const int tdx = hbm_clamp ((cdx >> shift) + x, -bw, w) - x, tdy = hbm_clamp ((cdy >> shift) + y, -bh, h) - y;
  uint32_t acc = 0;
  if (alive) {
    const int cx = x + tdx, cy = y + tdy;
    for (int r = rg; r < bh; r += 4) {
      const uint32_t *brow = block + r * nd;
      for (int d = 0; d < nd; d++) {
        uint32_t v = scan_fetch4 (lv.ref[0], lv.ref_stride[0], w, h, cx + 4 * d, cy + r);
        if (d == nd - 1)
          v &= tail;
        acc = __builtin_amdgcn_sad_u8 (v, brow[d], acc);
      }
    }
    const int hs = lv.hs, vs = lv.vs;
    const int pw = (w + (1 << hs) - 1) >> hs, ph = (h + (1 << vs) - 1) >> vs;    // ROUND_UP_SHIFT
    const int fx = x >> hs, fy = y >> vs;
    const int cw = min (pw - fx, xb >> hs), chh = min (ph - fy, yb >> vs);
    for (int k = 1; k < 3; k++)
      acc = hbm_chroma_sad (lv.frame[k], lv.frame_stride[k], lv.ref[k], lv.ref_stride[k], pw, ph, fx, fy, cx >> hs, cy >> vs, cw, chh, rg, acc);
  }
  acc += (uint32_t) __shfl_xor ((int) acc, 16);
  acc += (uint32_t) __shfl_xor ((int) acc, 32);
  uint32_t key = alive ? (acc << 4) | (uint32_t) c : 0xffffffffu;
  for (int off = 1; off < 16; off <<= 1)
    key = min (key, (uint32_t) __shfl_xor ((int) key, off));
  // (the last present entry is always alive: key names a slot; SCHRO_ASSERT (-1 < min_m))
  const int win = (int) (key & 15u);    // lane `win` holds slot `win`
  int gx = __shfl (cdx, win) >> shift, gy = __shfl (cdy, win) >> shift;
  gx = max (-bw - x, min (w - x, gx));  // :357-358
  gy = max (-bh - y, min (h - y, gy));

  // ---- the scan: the window holds the start vector, and a window without a position stores it ----
  // (ext >= max (xb, yb): 0 < sw, sh <= 2 * dist + 1 and the start vector lies inside; checked all the same -- a window
  // the LDS was not sized for is not staged)
  const ScanRules rules = { false, false, true, false };
  scan_and_store (lv, lv.ref[0], lv.ref_stride[0], w, h, shift, mv_record (lv.field, nbx, i, j), ref, x, y, bw, bh, gx, gy, block, window, rules, lane);
}

__global__ __launch_bounds__ (kChainThreads)
void hier_bm_kernel (const HbmChain * __restrict__ chains, int lds_per_wave)
{
  extern __shared__ __attribute__ ((aligned (16))) uint32_t hbm_lds[];
  const HbmChain *ch = chains + blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  uint32_t *lds = hbm_lds + (size_t) wave * (lds_per_wave >> 2);
  const int nbx = ch->nbx, nby = ch->nby, nlevels = ch->nlevels;

  // schro_motion_field_set (mf, split, ref + 1): pred_mode | split << 3
  const int ref = ch->ref;
  fill_fields (ch, [ref](const HbmLevel & lv) {
        return (uint32_t) (ref + 1) | ((lv.shift > 1 ? 0u : (lv.shift == 1 ? 1u : 2u)) << 3);
      });

  for (int n = 0; n < nlevels; n++) {
    const HbmLevel & lv = ch->level[n];   // (read where it is used: 32 scalars held across the block would spill)
    const int shift = lv.shift;
    const int cols = (nbx + (1 << shift) - 1) >> shift, rws = (nby + (1 << shift) - 1) >> shift;       // the level's grid
    walk_diagonals (cols, rws, wave, nwaves, [&](int bi, int bj) {
          hbm_block (ch, lv, bi << shift, bj << shift, lds, lane);
        });
  }
}

int
launch_hier_bm (hipStream_t stream, const HbmChain * d_chains, int nchains, size_t lds_per_wave)
{
  return launch_chains (hier_bm_kernel, "block matching", stream, d_chains, nchains, lds_per_wave);
}

}                               // namespace schro
