// scan_common.h -- the wave-level SAD scan (schro_metric_scan_do_scan + schro_metric_scan_get_min, schrometric.c:31-171)
// shared by metric_scan_kernel (analysis.hip) and, through scan_and_store of motion_common.h, rough_hint_kernel and hier_bm_kernel: the LDS layout of a wave's block
// and window, their staging, and the minimum over the window's positions.  analysis.hip describes the layout.
#pragma once

#include "schro_hip_internal.h"

namespace schro {

// bytes between the staged block's rows, the staged window's rows, and the window columns staged
__host__ __device__ __forceinline__ int
scan_block_pitch (int bw)
{
  return (bw + 3) & ~3;
}

// the window read of a position reaches (block dwords + 1) dwords from the dword its first column lies in
__host__ __device__ __forceinline__ int
scan_window_cols (int bw, int sw)
{
  return ((sw - 1) & ~3) + scan_block_pitch (bw) + 4;
}

__host__ __device__ __forceinline__ int
scan_window_pitch (int bw, int sw)
{
  const int cols = scan_window_cols (bw, sw);
  return (cols >> 2) & 1 ? cols : cols + 4;     // an odd number of dwords
}

// the mask of the block's last dword in a row
__device__ __forceinline__ uint32_t
scan_tail_mask (int bw)
{
  return bw & 3 ? (1u << (8 * (bw & 3))) - 1 : 0xffffffffu;
}

// four samples of row `row` from column x on, coordinates clamped to the w x h picture, as one little-endian dword
__device__ __forceinline__ uint32_t
scan_fetch4 (const uint8_t * plane, int stride, int w, int h, int x, int y)
{
  const uint8_t *row = plane + (size_t) min (max (y, 0), h - 1) * stride;
  if (x >= 0 && x + 3 <= w - 1)
    return gload < u32_u > (row + x);
  uint32_t v = 0;
  for (int n = 0; n < 4; n++)
    v |= (uint32_t) gload < uint8_t > (row + min (max (x + n, 0), w - 1)) << (8 * n);
  return v;
}

// the wave's block: `rows` rows of nd dwords from (x, y) of the frame, the last dword of a row masked to the block
__device__ __forceinline__ void
scan_stage_block (uint32_t * block, const uint8_t * frame, int stride, int w, int h, int x, int y, int nd, int rows, uint32_t tail,
    int lane)
{
  for (int n = lane; n < nd * rows; n += 64) {
    const int r = n / nd, c = n - r * nd;
    const uint32_t v = scan_fetch4 (frame, stride, w, h, x + 4 * c, y + r);
    block[n] = c == nd - 1 ? v & tail : v;
  }
}

// the wave's window: wrows rows of wcols dwords from (ref_x, ref_y) of the reference, wd dwords apart
__device__ __forceinline__ void
scan_stage_window (uint32_t * window, const uint8_t * ref, int stride, int w, int h, int ref_x, int ref_y, int wd, int wcols, int wrows,
    int lane)
{
  for (int n = lane; n < wcols * wrows; n += 64) {
    const int r = n / wcols, c = n - r * wcols;
    window[r * wd + c] = scan_fetch4 (ref, stride, w, h, ref_x + 4 * c, ref_y + r);
  }
}

// The wave-wide minimum of (metric << 11) | order over the npos = scan_width * sh positions p = i * sh + j: order 0 for
// the gravity position pg (kept unless a strictly smaller metric exists), 1 + p otherwise (i outer, j inner: the first of
// equal metrics wins).  table (or NULL): where the metrics go.  m_sh: div_magic (sh).
__device__ __forceinline__ uint32_t
scan_wave_min (const uint32_t * block, const uint32_t * window, int nd, int rows, int wd, uint32_t tail, int npos, int sh, uint32_t m_sh,
    int pg, uint32_t * table, int lane)
{
  uint32_t best = 0xffffffffu;
  for (int p = lane; p < npos; p += 64) {
    const int i = mdiv (p, sh, m_sh);
    const int j = p - i * sh;
    const uint32_t *wrow = window + j * wd + (i >> 2);
    const uint32_t *brow = block;
    const uint32_t phase = i & 3;
    uint32_t acc = 0;
    for (int r = 0; r < rows; r++) {
      uint32_t lo = wrow[0];
      for (int c = 0; c < nd; c++) {
        const uint32_t hi = wrow[c + 1];
        uint32_t v = __builtin_amdgcn_alignbyte (hi, lo, phase);
        if (c == nd - 1)
          v &= tail;
        acc = __builtin_amdgcn_sad_u8 (v, brow[c], acc);
        lo = hi;
      }
      wrow += wd;
      brow += nd;
    }
    if (table)
      gstore < uint32_t > (table + p, acc);
    best = min (best, (acc << 11) | (p == pg ? 0u : (uint32_t) (1 + p)));
  }
  for (int off = 32; off; off >>= 1)
    best = min (best, (uint32_t) __shfl_xor ((int) best, off));
  return best;
}

}                               // namespace schro
