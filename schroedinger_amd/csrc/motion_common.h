// motion_common.h -- what the encoder's motion stages share on the device (rough_hint.hip, hier_bm.hip, subpel.hip and,
// through mode_common.h, mode_split2.hip and mode_decision.hip): the SchroMotionVector record, the wave-level LDS fence,
// the entropy estimate and the vector prediction, the fetch from a tiled upsampled image, and -- for the two searches that
// run a chain of levels inside one launch -- the field-set preamble, the anti-diagonal walk, the scan around a start
// vector and the launch.  Nothing here is used by one file alone, and nothing here does floating point: the files that
// round scores twice switch contraction off themselves.
#pragma once

#include "schro_hip_internal.h"
#include "scan_common.h"

#include <algorithm>
#include <climits>

namespace schro {

// ---- the record (kMvBytes and the offsets: schro_hip_internal.h) ---------------------------------------------------------

// record (i, j) of a field nbx records wide
template < class Byte > __device__ __forceinline__ Byte *
mv_record (Byte * field, int nbx, int i, int j)
{
  return field + ((size_t) j * nbx + i) * kMvBytes;
}

// dx[ref], dy[ref] of a record
__device__ __forceinline__ void
mv_vector (const uint8_t * rec, int ref, int *vx, int *vy)
{
  *vx = gload < int16_t > (rec + kMvDx + 2 * ref);
  *vy = gload < int16_t > (rec + kMvDy + 2 * ref);
}

// neighbour k of block (i, j) -- 0: left, 1: above, 2: above-left, `skip` records away -- or NULL at the field's edge
__device__ __forceinline__ const uint8_t *
mv_neighbour (const uint8_t * field, int nbx, int i, int j, int skip, int k)
{
  if (k == 0)
    return i > 0 ? mv_record (field, nbx, i - skip, j) : nullptr;
  if (k == 1)
    return j > 0 ? mv_record (field, nbx, i, j - skip) : nullptr;
  return i > 0 && j > 0 ? mv_record (field, nbx, i - skip, j - skip) : nullptr;
}

// what the wave's lanes stored in LDS is read by other lanes of the same wave: LDS serves a wave's accesses in order, the
// compiler must not reorder them  (static: lowdelay.hip has a wave_sync of its own)
static __device__ __forceinline__ void
wave_sync ()
{
  __builtin_amdgcn_fence (__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier ();
  __builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the entropy estimate and the vector prediction ------------------------------------------------------------------------

// schro_pack_estimate_sint (schropack.c:204-226)
__device__ __forceinline__ int
estimate_sint (int value)
{
  const uint32_t a = (uint32_t) (value < 0 ? -value : value);
  const int n_bits = 32 - __clz ((int) (a + 1));        // maxbit (value + 1)
  return n_bits + n_bits - 1 + (a ? 1 : 0);
}

__device__ __forceinline__ int
median3 (int a, int b, int c)
{
  return max (min (a, b), min (max (a, b), c));
}

// whether a record -- its flags, dx[0] | dx[1] << 16, dy[0] | dy[1] << 16 -- predicts for `mode` (1 or 2: it is not intra
// and uses that reference), and its vector then
__device__ __forceinline__ bool
mv_predicts (uint32_t flags, uint32_t dx, uint32_t dy, int mode, int *vx, int *vy)
{
  if ((flags & 4) || !(flags & (uint32_t) mode))
    return false;
  *vx = (int16_t) (dx >> (16 * (mode - 1)));
  *vy = (int16_t) (dy >> (16 * (mode - 1)));
  return true;
}

// A source of neighbour records says whether record (x, y) predicts for a mode, and gives its vector.  This one: a field
// in global memory.
struct GlobalRecords {
  const uint8_t *field;
  int nbx;
  __device__ __forceinline__ void raw (int x, int y, uint32_t * flags, uint32_t * dx, uint32_t * dy) const
  {
    const uint8_t *mv = mv_record (field, nbx, x, y);
    *flags = gload < uint32_t > (mv + kMvFlags);
    *dx = gload < uint32_t > (mv + kMvDx);
    *dy = gload < uint32_t > (mv + kMvDy);
  }
  __device__ __forceinline__ bool operator () (int x, int y, int mode, int *vx, int *vy) const
  {
    uint32_t flags, dx, dy;
    raw (x, y, &flags, &dx, &dy);
    return mv_predicts (flags, dx, dy, mode, vx, vy);
  }
};

// schro_motion_vector_prediction (schromotion.c:315-368) for block (i, j), mode 1 or 2: left, above, above-left, those
// that predict; none: 0, one: itself, two: their rounded mean, three: the median
template < class Records > __device__ __forceinline__ void
vector_prediction (const Records & get, int i, int j, int mode, int *px, int *py)
{
  int vx[3], vy[3], n = 0;
  if (i > 0 && get (i - 1, j, mode, &vx[n], &vy[n]))
    n++;
  if (j > 0) {
    if (get (i, j - 1, mode, &vx[n], &vy[n]))
      n++;
    if (i > 0 && get (i - 1, j - 1, mode, &vx[n], &vy[n]))
      n++;
  }
  *px = 0, *py = 0;
  if (n == 1)
    *px = vx[0], *py = vy[0];
  else if (n == 2)
    *px = (vx[0] + vx[1] + 1) >> 1, *py = (vy[0] + vy[1] + 1) >> 1;
  else if (n == 3)
    *px = median3 (vx[0], vx[1], vx[2]), *py = median3 (vy[0], vy[1], vy[2]);
}

// ---- the tiled upsampled image ----------------------------------------------------------------------------------------------

// 16 samples of component `cb` from half-pel column X (and every second one after it) of half-pel row Y: the row is
// clamped to [0, 2 h - 2] and then selects its plane, the column is clamped to the image's aprons
__device__ __forceinline__ u32x4
tap (const uint8_t * up, int stride, int w, int h, int X, int Y, int pair, int cb)
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

// a position in units of mvprec as its half-pel origin and its remainder in eighths
__device__ __forceinline__ void
halfpel_split (int x, int y, int mvprec, int *hx, int *hy, int *rx, int *ry)
{
  *hx = x, *hy = y, *rx = 0, *ry = 0;
  if (mvprec == 0) {
    *hx = 2 * x, *hy = 2 * y;
  } else if (mvprec == 2) {
    *hx = x >> 1, *rx = (x & 1) << 1;
    *hy = y >> 1, *ry = (y & 1) << 1;
  } else if (mvprec == 3) {
    *hx = x >> 2, *rx = x & 3;
    *hy = y >> 2, *ry = y & 3;
  }
}

// 16 samples of the row whose first sample lies at half-pel (hx, hy) plus (rx, ry) eighths: (w00 S (hx, hy) + w01 S (hx +
// 1, hy) + w10 S (hx, hy + 1) + w11 S (hx + 1, hy + 1) + 8) >> 4 with the bilinear weights, which sum to 16, applied to
// the even and the odd bytes of a dword as two 16-bit halves each.  A tap of weight 0 is not fetched; weight 16 is the
// sample itself: one load.
__device__ __forceinline__ u32x4
predict_halfpel (const uint8_t * up, int stride, int w, int h, int hx, int hy, int rx, int ry, int pair, int cb)
{
  if ((rx | ry) == 0)
    return tap (up, stride, w, h, hx, hy, pair, cb);
  const uint32_t wt[4] = { (uint32_t) ((4 - ry) * (4 - rx)), (uint32_t) ((4 - ry) * rx), (uint32_t) (ry * (4 - rx)), (uint32_t) (ry * rx) };
  u32x4 even = { 0x00080008u, 0x00080008u, 0x00080008u, 0x00080008u }, odd = even;
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (wt[t]) {
      const u32x4 s = tap (up, stride, w, h, hx + (t & 1), hy + (t >> 1), pair, cb);
      even += (s & 0x00ff00ffu) * wt[t];
      odd += ((s >> 8) & 0x00ff00ffu) * wt[t];
    }
  return ((even >> 4) & 0x00ff00ffu) | (((odd >> 4) & 0x00ff00ffu) << 8);
}

// schro_upsampled_frame_get_block_fast_precN: 16 samples of the row whose first sample lies at (x, y) in units of mvprec
__device__ __forceinline__ u32x4
predict (const uint8_t * up, int stride, int w, int h, int x, int y, int mvprec, int pair, int cb)
{
  int hx, hy, rx, ry;
  halfpel_split (x, y, mvprec, &hx, &hy, &rx, &ry);
  return predict_halfpel (up, stride, w, h, hx, hy, rx, ry, pair, cb);
}

// ---- a chain of levels in one workgroup: rough_hint.hip, hier_bm.hip ---------------------------------------------------------

constexpr int kChainWaves = SCHRO_HIP_ROUGH_WAVES;
constexpr int kChainThreads = kChainWaves * 64;
constexpr size_t kChainLdsLimit = 65536;

// schro_motion_field_set on every field of the chain: five dwords per record, the first one flags (lv), the others 0
template < class Chain, class Flags > __device__ __forceinline__ void
fill_fields (const Chain * ch, const Flags & flags)
{
  const size_t records = (size_t) ch->nbx * ch->nby;
  for (int n = 0; n < ch->nlevels; n++) {
    uint8_t *field = ch->level[n].field;
    const uint32_t first = flags (ch->level[n]);
    for (size_t k = threadIdx.x; k < records; k += blockDim.x)
      for (int m = 0; m < kMvBytes / 4; m++)
        gstore < uint32_t > (field + k * kMvBytes + 4 * m, m == 0 ? first : 0u);
  }
  __syncthreads ();
}

// The anti-diagonals d = i + j of a cols x rws grid, one after the other: block (d - j, j) of a diagonal goes to
// block (i, j) on the thread, or wave, for which j = first, first + stride, .. from the diagonal's top; __syncthreads ()
// separates the diagonals -- the next one reads this one's records.  Every thread of the workgroup comes here.
template < class Block > __device__ __forceinline__ void
walk_diagonals (int cols, int rws, int first, int stride, const Block & block)
{
  for (int d = 0; d < cols + rws - 1; d++) {
    const int jlo = max (0, d - (cols - 1)), jhi = min (d, rws - 1);
    for (int j = jlo + first; j <= jhi; j += stride)
      block (d - j, j);
    __syncthreads ();
  }
}

// what the two searches do differently around the scan
struct ScanRules {
  bool first_is_gravity;        // the window's first position becomes the start vector (the rough nohint level)
  bool zero_without_window;     // a window without a position stores 0, 0 -- else the start vector -- and INT_MAX
  bool bounded;                 // a window over 2 * dist + 1 wide or high is one without a position
  bool empty;                   // a block of no width or height: the start vector is kept with metric 0, nothing is staged
};

// The scan of a bw x bh block at (x, y) of level lv (its dist and ext; the caller holds w, h and shift; ref_plane,
// ref_stride: its reference's luma) around the start vector (gx, gy): the window of schro_metric_scan_setup (schrometric.c:174-214), staged behind the
// staged block, the minimum of scan_wave_min with the start vector as gravity, and metric, dx[ref], dy[ref] << shift into
// `out`.
template < class Level > __device__ __forceinline__ void
scan_and_store (const Level & lv, const uint8_t * ref_plane, int ref_stride, int w, int h, int shift, uint8_t * out, int ref, int x, int y, int bw,
    int bh, int gx, int gy, const uint32_t * block, uint32_t * window, const ScanRules & rules, int lane)
{
  const int dist = lv.dist, ext = lv.ext;       // (read here, where they are used: hier_bm.hip says why)
  const int ref_x = max (max (-bw, x + gx - dist), -ext), ref_y = max (max (-bh, y + gy - dist), -ext);
  const int sw = min (min (w, x + gx + dist), w - bw + ext) - ref_x + 1;
  const int sh = min (min (h, y + gy + dist), h - bh + ext) - ref_y + 1;
  if (rules.first_is_gravity) {
    gx = ref_x - x;
    gy = ref_y - y;
  }
  int dx = gx, dy = gy;
  uint32_t metric = (uint32_t) INT_MAX; // SCHRO_METRIC_INVALID
  if (sw <= 0 || sh <= 0 || (rules.bounded && (sw > 2 * dist + 1 || sh > 2 * dist + 1))) {
    if (rules.zero_without_window)
      dx = dy = 0;
  } else if (rules.empty) {
    metric = 0;
  } else {
    const int nd = scan_block_pitch (bw) >> 2;
    const uint32_t tail = scan_tail_mask (bw);
    const int wd = scan_window_pitch (bw, sw) >> 2, wcols = scan_window_cols (bw, sw) >> 2;
    scan_stage_window (window, ref_plane, ref_stride, w, h, ref_x, ref_y, wd, wcols, bh + sh - 1, lane);
    wave_sync ();
    const uint32_t m_sh = sh > 1 ? kDivMagic.m[sh] : 0u;
    const uint32_t best = scan_wave_min (block, window, nd, bh, wd, tail, sw * sh, sh, m_sh, (gx + x - ref_x) * sh + (gy + y - ref_y), nullptr, lane);
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
    gstore < uint32_t > (out + kMvMetric, metric);
    gstore < uint16_t > (out + kMvDx + 2 * ref, (uint16_t) ((uint32_t) dx << shift));
    gstore < uint16_t > (out + kMvDy + 2 * ref, (uint16_t) ((uint32_t) dy << shift));
  }
}

// one workgroup per chain, as many waves as the workgroup's LDS holds, kChainWaves at the most and at least one
template < class Chain > int
launch_chains (void (*kernel) (const Chain *, int), const char *who, hipStream_t stream, const Chain * d_chains, int nchains, size_t lds_per_wave)
{
  if (lds_per_wave > kChainLdsLimit)
    return set_error (SCHRO_HIP_EINVAL, "%s launch: %zu bytes of LDS per wave", who, lds_per_wave);
  const int waves = lds_per_wave ? (int) std::min < size_t > (kChainWaves, kChainLdsLimit / lds_per_wave) : kChainWaves;
  SCHRO_LAUNCH (kernel, dim3 (nchains), dim3 (waves * 64), lds_per_wave * waves, stream, d_chains, (int) lds_per_wave);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "%s launch: %s", who, hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
