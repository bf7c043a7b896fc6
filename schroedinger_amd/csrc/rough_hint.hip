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

#include "schro_hip_internal.h"
#include "scan_common.h"

#include <algorithm>
#include <climits>

namespace schro {

constexpr int kRoughWaves = SCHRO_HIP_ROUGH_WAVES;
constexpr int kRoughThreads = kRoughWaves * 64;
constexpr size_t kRoughLdsLimit = 65536;
constexpr int kMvBytes = 20;    // SchroMotionVector (schromotion.h:20-37): flags, metric, chroma_metric, dx[2], dy[2]
constexpr int kMvMetric = 4, kMvDx = 12, kMvDy = 16;

// what the wave's lanes stored in LDS is read by other lanes of the same wave: LDS serves a wave's accesses in order, the
// compiler must not reorder them
__device__ __forceinline__ void
rough_wave_sync ()
{
  __builtin_amdgcn_fence (__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier ();
  __builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "wavefront");
}

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

  rough_wave_sync ();           // (the block before this one is through with the LDS)
  scan_stage_block (block, lv.frame, lv.frame_stride, w, h, x, y, nd, rows, tail, lane);
  rough_wave_sync ();

  int gx = 0, gy = 0;           // the scan's vector: the winner >> shift
  if (lv.hint) {
    const int c = lane & 7;
    const int mask = ~((1 << (shift + 1)) - 1);
    const uint8_t *rec = nullptr;
    if (c >= 1 && c <= 4) {
      const int m = c - 1;
      const int l = (i + skip * (-1 + 2 * (m & 1))) & mask, k = (j + skip * (-1 + (m & 2))) & mask;    // negative stays negative
      if (l >= 0 && l < nbx && k >= 0 && k < nby)
        rec = lv.hint + ((size_t) k * nbx + l) * kMvBytes;
    } else if (c == 5) {
      if (i > 0)
        rec = lv.field + ((size_t) j * nbx + (i - skip)) * kMvBytes;
    } else if (c == 6) {
      if (j > 0)
        rec = lv.field + ((size_t) (j - skip) * nbx + i) * kMvBytes;
    } else if (c == 7) {
      if (i > 0 && j > 0)
        rec = lv.field + ((size_t) (j - skip) * nbx + (i - skip)) * kMvBytes;
    }
    int cdx = 0, cdy = 0;
    if (rec) {
      cdx = gload < int16_t > (rec + kMvDx + 2 * ref);
      cdy = gload < int16_t > (rec + kMvDy + 2 * ref);
    }
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

  // schro_metric_scan_setup (schrometric.c:174-214)
  const int dist = lv.dist, ext = lv.ext;
  const int ref_x = max (max (-bw, x + gx - dist), -ext), ref_y = max (max (-bh, y + gy - dist), -ext);
  const int sw = min (min (w, x + gx + dist), w - bw + ext) - ref_x + 1;
  const int sh = min (min (h, y + gy + dist), h - bh + ext) - ref_y + 1;
  if (!lv.hint) {               // :106-109: the gravity of the nohint level is the window's first position
    gx = ref_x - x;
    gy = ref_y - y;
  }
  int dx = gx, dy = gy;
  uint32_t metric = 0;
  if (sw <= 0 || sh <= 0) {
    dx = dy = 0;
    metric = (uint32_t) INT_MAX;        // SCHRO_METRIC_INVALID
  } else if (!empty) {
    const int wd = scan_window_pitch (bw, sw) >> 2, wcols = scan_window_cols (bw, sw) >> 2;
    scan_stage_window (window, lv.ref, lv.ref_stride, w, h, ref_x, ref_y, wd, wcols, rows + sh - 1, lane);
    rough_wave_sync ();
    const uint32_t m_sh = sh > 1 ? kDivMagic.m[sh] : 0u;
    const uint32_t best = scan_wave_min (block, window, nd, rows, wd, tail, sw * sh, sh, m_sh, (gx + x - ref_x) * sh + (gy + y - ref_y), nullptr, lane);
    metric = best >> 11;
    const uint32_t order = best & 2047u;
    if (order) {
      const int p = (int) order - 1;
      const int pi = mdiv (p, sh, m_sh);
      dx = ref_x + pi - x;
      dy = ref_y + (p - pi * sh) - y;
    }
  }
  if (lane == 0) {
    uint8_t *out = lv.field + ((size_t) j * nbx + i) * kMvBytes;
    gstore < uint32_t > (out + kMvMetric, metric);
    gstore < uint16_t > (out + kMvDx + 2 * ref, (uint16_t) ((uint32_t) dx << shift));
    gstore < uint16_t > (out + kMvDy + 2 * ref, (uint16_t) ((uint32_t) dy << shift));
  }
}

__global__ __launch_bounds__ (kRoughThreads)
void rough_hint_kernel (const RoughChain * __restrict__ chains, int lds_per_wave)
{
  extern __shared__ __attribute__ ((aligned (16))) uint32_t rough_lds[];
  const RoughChain *ch = chains + blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  uint32_t *lds = rough_lds + (size_t) wave * (lds_per_wave >> 2);
  const int nbx = ch->nbx, nby = ch->nby, nlevels = ch->nlevels;

  // schro_motion_field_set (mf, 0, 1) on every field: five dwords per record, the first one 1
  const size_t records = (size_t) nbx * nby;
  for (int n = 0; n < nlevels; n++) {
    uint8_t *field = ch->level[n].field;
    for (size_t k = threadIdx.x; k < records; k += blockDim.x)
      for (int m = 0; m < kMvBytes / 4; m++)
        gstore < uint32_t > (field + k * kMvBytes + 4 * m, m == 0 ? 1u : 0u);
  }
  __syncthreads ();

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
    for (int d = 0; d < cols + rws - 1; d++) {
      const int jlo = max (0, d - (cols - 1)), jhi = min (d, rws - 1);
      for (int bj = jlo + wave; bj <= jhi; bj += nwaves)
        rough_block (ch, lv, (d - bj) << shift, bj << shift, lds, lane);
      __syncthreads ();         // the next diagonal reads this one's records
    }
  }
}

int
launch_rough_hint (hipStream_t stream, const RoughChain * d_chains, int nchains, size_t lds_per_wave)
{
  if (lds_per_wave > kRoughLdsLimit)
    return set_error (SCHRO_HIP_EINVAL, "rough search launch: %zu bytes of LDS per wave", lds_per_wave);
  // as many waves as the workgroup's LDS holds, and at least one
  const int waves = lds_per_wave ? (int) std::min < size_t > (kRoughWaves, kRoughLdsLimit / lds_per_wave) : kRoughWaves;
  SCHRO_LAUNCH (rough_hint_kernel, dim3 (nchains), dim3 (waves * 64), lds_per_wave * waves, stream, d_chains, (int) lds_per_wave);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "rough search launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
