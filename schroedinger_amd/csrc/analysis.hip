// analysis.hip -- encoder analysis: the downsample pyramid (schro_frame_downsample + schro_frame_mc_edgeextend,
// schroframe.c:1449-1505, :1940-1997) and the SAD scan (schro_metric_scan_do_scan + schro_metric_scan_get_min,
// schrometric.c:31-171).  Integer arithmetic only: both are bit-exact against the reference.

#include "schro_hip_internal.h"
#include "scan_common.h"

namespace schro {

// ---- downsample ------------------------------------------------------------------------------------------------------
//
// A workgroup of 4 waves owns a tile of 256 columns x 8 rows of the destination INCLUDING its apron; a wave takes a row
// at a time, a lane a group of 4 adjacent destination bytes.  A group inside the picture loads 8 source bytes of each of
// the four (clamped) source rows, filters the columns to 8 u8 samples held in two registers (the reference's first
// rounding), takes the two samples beside them from the neighbouring lanes (or filters them itself at the ends of the
// wave and of the picture), filters along the row and stores one dword.  Every other group -- the apron, the picture's
// last columns -- is computed sample by sample at its clamped coordinate: nothing the launch writes is read.

constexpr int kDownThreads = 256;
constexpr int kDownTileCols = 256;      // 64 lanes x 4 bytes
constexpr int kDownTileRows = 8;        // 4 waves x 2 rows

// (6 (a + d) + 26 (b + c) + 32) >> 6 on four packed u8 samples: two 16-bit fields per register, at most 16352 each
__device__ __forceinline__ uint32_t
down_filter_packed (uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  const uint32_t m = 0x00ff00ffu;
  const uint32_t e = 6 * ((a & m) + (d & m)) + 26 * ((b & m) + (c & m)) + 0x00200020u;
  const uint32_t o = 6 * (((a >> 8) & m) + ((d >> 8) & m)) + 26 * (((b >> 8) & m) + ((c >> 8) & m)) + 0x00200020u;
  return ((e >> 6) & m) | (((o >> 6) & m) << 8);
}

__device__ __forceinline__ uint32_t
down_filter (uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  return (6 * (a + d) + 26 * (b + c) + 32) >> 6;
}

// the column filter's u8 result at source column x (inside the picture) of the four source rows
__device__ __forceinline__ uint32_t
down_vert_sample (const uint8_t * r0, const uint8_t * r1, const uint8_t * r2, const uint8_t * r3, int x)
{
  return down_filter (gload < uint8_t > (r0 + x), gload < uint8_t > (r1 + x), gload < uint8_t > (r2 + x), gload < uint8_t > (r3 + x));
}

__global__ __launch_bounds__ (kDownThreads)
void downsample_kernel (const DownsampleJob * __restrict__ jobs, int njobs)
{
  const int bid = blockIdx.x;
  const DownsampleJob job = jobs[find_job (jobs, njobs, bid)];
  const int t = bid - job.tile_base;
  const int ty = mdiv (t, job.tiles_x, job.m_tiles_x);
  const int tx = t - ty * job.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sw = job.sw, sh = job.sh, dw = job.dw, dh = job.dh, ext = job.ext;

  const int x0 = job.xorg + tx * kDownTileCols + lane * 4;      // this lane's four destination columns x0 .. x0 + 3
  // a group all of whose samples, and all of whose 8 source columns, lie inside the picture
  const bool fast = x0 >= 0 && x0 + 3 <= dw - 1 && 2 * x0 + 7 <= sw - 1;
  const bool left_fast = lane > 0 && x0 - 4 >= 0;               // (then the lane to the left is fast too)
  const bool right_fast = lane < 63 && x0 + 7 <= dw - 1 && 2 * x0 + 15 <= sw - 1;

  for (int k = 0; k < kDownTileRows / 4; k++) {
    const int y = -ext + ty * kDownTileRows + wave * (kDownTileRows / 4) + k;   // wave-uniform
    if (y >= dh + ext)
      break;
    const int cy = min (max (y, 0), dh - 1);
    const uint8_t *r0 = job.src + (size_t) max (2 * cy - 1, 0) * job.src_stride;
    const uint8_t *r1 = job.src + (size_t) min (2 * cy, sh - 1) * job.src_stride;
    const uint8_t *r2 = job.src + (size_t) min (2 * cy + 1, sh - 1) * job.src_stride;
    const uint8_t *r3 = job.src + (size_t) min (2 * cy + 2, sh - 1) * job.src_stride;
    uint8_t *out = job.dst + (ptrdiff_t) y * job.dst_stride;

    uint32_t lo = 0, hi = 0;
    if (fast) {
      const u32x2 a = gload < u32x2_u > (r0 + 2 * x0), b = gload < u32x2_u > (r1 + 2 * x0);
      const u32x2 c = gload < u32x2_u > (r2 + 2 * x0), d = gload < u32x2_u > (r3 + 2 * x0);
      lo = down_filter_packed (a.x, b.x, c.x, d.x);
      hi = down_filter_packed (a.y, b.y, c.y, d.y);
    }
    // the samples beside the eight: the left neighbour's last, the right neighbour's first (every lane takes part)
    uint32_t left = __shfl_up (hi >> 24, 1);
    uint32_t right = __shfl_down (lo & 255, 1);
    if (fast) {
      if (!left_fast)
        left = down_vert_sample (r0, r1, r2, r3, max (2 * x0 - 1, 0));
      if (!right_fast)
        right = down_vert_sample (r0, r1, r2, r3, min (2 * x0 + 8, sw - 1));
      const uint32_t t0 = lo & 255, t1 = (lo >> 8) & 255, t2 = (lo >> 16) & 255, t3 = lo >> 24;
      const uint32_t t4 = hi & 255, t5 = (hi >> 8) & 255, t6 = (hi >> 16) & 255, t7 = hi >> 24;
      const uint32_t v = down_filter (left, t0, t1, t2) | (down_filter (t1, t2, t3, t4) << 8)
          | (down_filter (t3, t4, t5, t6) << 16) | (down_filter (t5, t6, t7, right) << 24);
      gstore < u32_u > (out + x0, v);
    } else {
      for (int n = 0; n < 4; n++) {
        const int x = x0 + n;
        if (x < -ext || x >= dw + ext)
          continue;
        const int cx = min (max (x, 0), dw - 1);
        const uint32_t a = down_vert_sample (r0, r1, r2, r3, max (2 * cx - 1, 0));
        const uint32_t b = down_vert_sample (r0, r1, r2, r3, min (2 * cx, sw - 1));
        const uint32_t c = down_vert_sample (r0, r1, r2, r3, min (2 * cx + 1, sw - 1));
        const uint32_t d = down_vert_sample (r0, r1, r2, r3, min (2 * cx + 2, sw - 1));
        gstore < uint8_t > (out + x, (uint8_t) down_filter (a, b, c, d));
      }
    }
  }
}

void
downsample_tile_geometry (int *cols, int *rows)
{
  *cols = kDownTileCols;
  *rows = kDownTileRows;
}

int
launch_downsample (hipStream_t stream, const DownsampleJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH (downsample_kernel, dim3 (total_tiles), dim3 (kDownThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "downsample launch: %s", hipGetErrorString (e));
  return 0;
}

// ---- SAD scan --------------------------------------------------------------------------------------------------------
//
// (The LDS layout, the staging and the minimum are in scan_common.h: rough_hint.hip runs the same scan per block.)
//
// One wave per scan, four scans per workgroup.  The wave stages its block (rows padded with zeros to whole dwords) and
// the reference window the scan touches -- (block_width + scan_width - 1) x (block_height + scan_height - 1) samples at
// clamped coordinates: the edge-extended apron -- in its share of the LDS, then its lanes take positions p = i *
// scan_height + j in turn: v_sad_u8 over the block's dwords, the window's dwords brought to the position's byte phase
// with v_alignbyte.  Neighbouring lanes differ in j, a window row apart: the row pitch is an odd number of dwords, so
// they read different banks; the block's dwords are the same address for every lane (a broadcast).
// The minimum keeps the reference's order of ties exactly: a wave-wide minimum of (metric << 11) | order, order 0 for the
// gravity position (the scan's starting minimum, which only a strictly smaller metric replaces) and 1 + p otherwise (i
// outer, j inner: the first of equal metrics wins).  metric <= 64 * 64 * 255 < 2^20, order <= 42 * 42 < 2^11.

constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;
constexpr size_t kScanLdsLimit = 65536;

size_t
scan_lds_bytes (int bw, int bh, int sw, int sh)
{
  if (bw <= 0 || bh <= 0)
    return 0;
  return round_up ((size_t) scan_block_pitch (bw) * bh + (size_t) scan_window_pitch (bw, sw) * (bh + sh - 1), 16);
}

size_t
scan_lds_limit ()
{
  return kScanLdsLimit / kScanWaves;
}

__global__ __launch_bounds__ (kScanThreads)
void metric_scan_kernel (const ScanPicture * __restrict__ pics, const ScanJob * __restrict__ scans, int nscans, int lds_per_wave)
{
  extern __shared__ __attribute__ ((aligned (16))) uint32_t scan_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sid = blockIdx.x * kScanWaves + wave;       // wave-uniform
  const bool active = sid < nscans;
  const ScanJob s = scans[active ? sid : 0];
  const ScanPicture pic = pics[s.pic];
  const bool empty = s.bw <= 0 || s.bh <= 0;
  const int nd = empty ? 0 : scan_block_pitch (s.bw) >> 2;      // dwords per block row
  const int rows = empty ? 0 : s.bh;
  const int wd = scan_window_pitch (s.bw, s.sw) >> 2;           // dwords per staged window row
  const int wcols = scan_window_cols (s.bw, s.sw) >> 2;         // ... of which are staged
  const int wrows = rows ? rows + s.sh - 1 : 0;
  uint32_t *block = scan_lds + (size_t) wave * (lds_per_wave >> 2);
  uint32_t *window = block + nd * rows;

  const uint32_t tail = scan_tail_mask (s.bw);
  if (active) {
    scan_stage_block (block, pic.frame, pic.frame_stride, pic.width, pic.height, s.x, s.y, nd, rows, tail, lane);
    scan_stage_window (window, pic.ref, pic.ref_stride, pic.width, pic.height, s.ref_x, s.ref_y, wd, wcols, wrows, lane);
  }
  __syncthreads ();
  if (!active)
    return;

  uint32_t *table = pic.metrics ? pic.metrics + (size_t) (sid - pic.scan_base) * (SCHRO_HIP_LIMIT_METRIC_SCAN * SCHRO_HIP_LIMIT_METRIC_SCAN) : nullptr;
  const uint32_t best = scan_wave_min (block, window, nd, rows, wd, tail, s.sw * s.sh, s.sh, s.m_sh, s.gi * s.sh + s.gj, table, lane);
  if (lane == 0) {
    const uint32_t order = best & 2047u;
    int dx = s.dx, dy = s.dy;
    if (order) {
      const int p = (int) order - 1;
      const int i = mdiv (p, s.sh, s.m_sh);
      dx = s.ref_x + i - s.x;
      dy = s.ref_y + (p - i * s.sh) - s.y;
    }
    u32x4 out;
    out.x = (uint32_t) dx;
    out.y = (uint32_t) dy;
    out.z = best >> 11;
    out.w = 0;
    gstore < u32x4 > (pic.results + (sid - pic.scan_base), out);
  }
}

int
launch_metric_scan (hipStream_t stream, const ScanPicture * d_pics, const ScanJob * d_scans, int nscans, size_t lds_per_wave)
{
  if (lds_per_wave > scan_lds_limit ())
    return set_error (SCHRO_HIP_EINVAL, "metric scan launch: %zu bytes of LDS per scan", lds_per_wave);
  SCHRO_LAUNCH (metric_scan_kernel, dim3 (div_up (nscans, kScanWaves)), dim3 (kScanThreads), lds_per_wave * kScanWaves, stream,
      d_pics, d_scans, nscans, (int) lds_per_wave);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "metric scan launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
