// iwt_fwd.hip -- one level of the 2-D FORWARD integer lifting wavelet, all seven Dirac
// filters, s16 and s32, for gfx950: the mirror of iiwt.hip's iiwt_level_kernel.
//
// What it computes: schro_wavelet_transform_2d (schroedinger/schrowaveletorc.c:60-120) for one
// level view, i.e. schro_iwt_desl_9_3, _5_3, _13_5, _haar0/1, _fidelity, _daub_9_7 and their
// _s32 twins (:285-1458), with the kernel arithmetic of schroedinger/schroorc.orc (16-bit wrap
// points for s16, 32-bit wrap for s32).  In lifting terms: the synthesis steps of iiwt_steps.h
// in reverse order with the opposite sign -- per row the deinterleave (with the << 1 of
// orc_deinterleave2_lshift1_* where the filter has an output shift) and the horizontal steps,
// then the vertical steps over even rows (low) and odd rows (high); out-of-range neighbours
// clamp inside the same half, what extend_N_M and the CLAMP (row, ...) rules produce.
//
// How: the level is cut into tiles; one 256-thread workgroup owns one tile and keeps the tile
// PLUS its lifting halo in LDS as [row][low half | high half].
//   * the source rows of the region are fetched with 8-byte coalesced loads (all loads of a
//     thread are issued before the first LDS write), shifted and split into the two halves;
//   * every lifting step is an in-place LDS pass: horizontal steps on sample quads of one
//     row, vertical steps on column quads of a row pair (one 64/128-bit LDS access);
//   * the last vertical step hands the updated row and its partner row straight to the four
//     sub-bands of the reference's in-place layout (even rows [LL | HL], odd rows [LH | HH]
//     of the level view), 8/16-byte stores.
// The level reads a compact image (the source plane, or the LL image the level before left
// in the scratch), writes its three detail bands into the coefficient frame and its LL band
// into the scratch (the last level: into the frame): nothing is in place, so tiles never race.
//
// Level 0 of an intra picture can read a PACKED picture instead (iwt_fwd_packed_kernel, schro_hip_unpack_iwt_batch): the
// same tile, LDS and lifting passes behind a staging stage that fetches the packed rows (unpack_fetch.h).  Measured it is
// bound by that stage's per-sample extraction, not by bytes.
//
// Bound: HBM.  Algorithmic bytes per input sample per level: 2 * sizeof(T).
// Open item: a register-tile form like iiwt_reg.hip's.

#include "schro_hip_internal.h"
#include "iiwt_steps.h"
#include "unpack_fetch.h"

namespace schro {
namespace {

constexpr int kThreads = 256;

// fidelity taps: stage 1 (c == 0) and stage 2 (c == 1), schrowaveletorc.c:606-623
__device__ constexpr int
fid_tap (int which, int k)
{
  constexpr int s1[8] = { -2, 10, -25, 81, 81, -25, 10, -2 };
  constexpr int s2[8] = { 8, -21, 46, -161, -161, 46, -21, 8 };
  return which ? s2[k] : s1[k];
}

// the widths of the Orc programs' intermediates (schroorc.orc): s16 pair sums wrap to 16 bits before the
// widening multiply, products and rounding in 32 bits; s32 wraps at 32 bits everywhere; avgs* never wrap
template < typename T > struct Ar;
template <> struct Ar < int16_t > {
  typedef int16_t T;
  static __device__ __forceinline__ T wrap (int v) { return (T) v; }
  static __device__ __forceinline__ int mul (T a, int c) { return (int) a * c; }
  static __device__ __forceinline__ int add32 (int a, int b) { return a + b; }
  static __device__ __forceinline__ int sub32 (int a, int b) { return a - b; }
  static __device__ __forceinline__ T avg (T a, T b) { return (T) (((int) a + (int) b + 1) >> 1); }
};
template <> struct Ar < int32_t > {
  typedef int32_t T;
  static __device__ __forceinline__ T wrap (int v) { return v; }
  static __device__ __forceinline__ int mul (T a, int c) { return (int) ((unsigned) a * (unsigned) c); }
  static __device__ __forceinline__ int add32 (int a, int b) { return (int) ((unsigned) a + (unsigned) b); }
  static __device__ __forceinline__ int sub32 (int a, int b) { return (int) ((unsigned) a - (unsigned) b); }
  static __device__ __forceinline__ T avg (T a, T b) { return (T) (((long long) a + (long long) b + 1) >> 1); }
};

// value of the lifting term of synthesis step K from its neighbours (schroorc.orc's opcode lists)
template < typename T, int F, int K >
__device__ __forceinline__ T
lift_term (const T * s)
{
  typedef Ar < T > A;
  constexpr Step st = filter_step (F, K);
  if constexpr (st.kind == K_ADD2_22) {
    T t = A::wrap (A::add32 (s[0], s[1]));
    t = A::wrap (A::add32 (t, 2));
    return (T) (t >> 2);
  } else if constexpr (st.kind == K_AVG11) {
    return A::avg (s[0], s[1]);
  } else if constexpr (st.kind == K_MAS4) {
    T t1 = A::wrap (A::add32 (s[1], s[2]));
    int t3 = A::mul (t1, 9);
    T t2 = A::wrap (A::add32 (s[0], s[3]));
    t3 = A::sub32 (t3, t2);
    t3 = A::add32 (t3, st.rnd);
    t3 >>= st.sh;
    return A::wrap (t3);
  } else if constexpr (st.kind == K_HAAR_HALF) {
    return A::avg (s[0], 0);
  } else if constexpr (st.kind == K_HAAR_FULL) {
    return s[0];
  } else if constexpr (st.kind == K_MAS8) {
    int x = st.rnd;
#pragma unroll
    for (int k = 0; k < 8; k++)
      x = A::add32 (x, A::mul (s[k], fid_tap (st.c, k)));
    return A::wrap (x >> 8);
  } else {
    T t1 = A::wrap (A::add32 (s[0], s[1]));
    int t2 = A::mul (t1, st.c);
    t2 = A::add32 (t2, st.rnd);
    t2 >>= st.sh;
    return A::wrap (t2);
  }
}

// the analysis direction of synthesis step K: the same term, the opposite sign
template < typename T, int F, int K >
__device__ __forceinline__ T
fwd_apply (T d, const T * s)
{
  typedef Ar < T > A;
  constexpr Step st = filter_step (F, K);
  T t = lift_term < T, F, K > (s);
  if constexpr (st.sign > 0)
    return A::wrap (A::sub32 (d, t));
  else
    return A::wrap (A::add32 (d, t));
}

// The tile: the inverse LDS form's (iiwt.hip Geo).  The halo of a filter is the sum of its steps' reaches, which
// does not depend on the order the steps run in.
template < typename T, int F > struct FwdGeo {
  static constexpr int RP = 32;                         // region row pairs
  static constexpr int H = filter_halo (F);
  static constexpr int HC = (H + 3) & ~3;               // keeps 8-byte alignment of loads and whole quads
  static constexpr int UC = sizeof (T) == 2 ? 128 : 64; // useful columns per half: whole 128-byte lines per band row
  static constexpr int RC = UC + 2 * HC;                // region columns per half
  static constexpr int UR = RP - 2 * H;                 // useful row pairs per tile
};

__device__ __forceinline__ int
clampi (int x, int lo, int hi)
{
  return min (max (x, lo), hi);
}

constexpr int
cmax (int a, int b)
{
  return a > b ? a : b;
}

constexpr int
floor4 (int a)
{
  return a >= 0 ? a / 4 * 4 : -((-a + 3) / 4 * 4);
}

// ---- staging: the region's source rows, 8 bytes = PL column pairs per load ------------------------------------
// (coordinates clamped into the picture; cells outside it are never read back)
template < typename T, int RP, int RC, int NPS >
__device__ __forceinline__ void
rows_load (uint2 * v, const void *base_, int stride, int tid, int r0, int c0, int nr, int nc)
{
  constexpr int PL = 4 / sizeof (T), NG = RC / PL;
  const char *base = (const char *) base_;
#pragma unroll
  for (int n = 0; n < NPS; n++) {
    const int it = min (tid + n * kThreads, 2 * RP * NG - 1);
    const int g = it % NG;
    const int y = it / NG;
    const int rr = clampi (2 * r0 + y, 0, 2 * nr - 1);
    const int c = clampi (c0 + g * PL, 0, nc - PL);
    const u32x2 q = gload < u32x2 > (base + (size_t) rr * stride + (size_t) c * 2 * sizeof (T));
    v[n] = make_uint2 (q.x, q.y);
  }
}

// the same region out of a packed picture's rows (unpack_fetch.h), in the layout an 8-byte load of the plane gives:
// sample coordinates clamped to the picture (xmax, ymax: the edge extension), the component extracted, the format's
// offset removed (u8: - 128; v210's - 512 and AY64's - 32768 are the unpack's own), the depth brought to T
template < typename T, int RP, int RC, int NPS >
__device__ __forceinline__ void
rows_load_packed (uint2 * v, const IwtFwdPackedJob & job, int tid, int r0, int c0, int nr, int nc)
{
  constexpr int PL = 4 / sizeof (T), NG = RC / PL;
  RowWords rw;
  rw.row = nullptr;
  rw.q = -1;
  rw.w = (u32x4) { 0, 0, 0, 0 };
  // (the source kind is uniform per workgroup: a scalar switch)
  unpack_by_kind (job.s.kind, [&](auto kind) {
#pragma unroll
    for (int n = 0; n < NPS; n++) {
      const int it = min (tid + n * kThreads, 2 * RP * NG - 1);
      const int g = it % NG;
      const int y = it / NG;
      const int rr = min (clampi (2 * r0 + y, 0, 2 * nr - 1), job.ymax);
      const uint8_t *row = job.s.base + (size_t) rr * job.s.stride;
      uint32_t a[2 * PL];
#pragma unroll
      for (int i = 0; i < 2 * PL; i++) {
        const int x = min (clampi (2 * (c0 + g * PL) + i, 0, 2 * nc - 1), job.xmax);
        a[i] = (uint32_t) unpack_depth (unpack_sample < decltype (kind)::value > (rw, job.s, row, x), job.s.depth, (int) sizeof (T));
      }
      if constexpr (sizeof (T) == 2)
        v[n] = make_uint2 ((a[0] & 0xffffu) | (a[1] << 16), (a[2] & 0xffffu) | (a[3] << 16));
      else
        v[n] = make_uint2 (a[0], a[1]);
    }
  });
}

// ... into LDS: even samples to the low half, odd samples to the high half, << 1 (wrapping: orc_deinterleave2_lshift1_*)
// where the filter has an output shift
template < typename T, int RP, int RC, int NPS, int SH >
__device__ __forceinline__ void
rows_store (T (*lds)[2 * RC], const uint2 * v, int tid)
{
  constexpr int PL = 4 / sizeof (T), NG = RC / PL;
#pragma unroll
  for (int n = 0; n < NPS; n++) {
    const int it = tid + n * kThreads;
    if (it < 2 * RP * NG) {
      const int g = it % NG;
      const int y = it / NG;
      uint32_t a, b;
      if constexpr (sizeof (T) == 2) {
        a = (v[n].x & 0xffffu) | (v[n].y << 16);
        b = (v[n].x >> 16) | (v[n].y & 0xffff0000u);
        if constexpr (SH != 0) {
          a = (a & 0x7fff7fffu) << 1;
          b = (b & 0x7fff7fffu) << 1;
        }
      } else {
        a = v[n].x << (SH != 0 ? 1 : 0);
        b = v[n].y << (SH != 0 ? 1 : 0);
      }
      *reinterpret_cast < uint32_t * >(&lds[y][g * PL]) = a;
      *reinterpret_cast < uint32_t * >(&lds[y][RC + g * PL]) = b;
    }
  }
}

template < typename T, int RP, int RC >
constexpr int
rows_nps ()
{
  return (2 * RP * (RC / (4 / (int) sizeof (T))) + kThreads - 1) / kThreads;
}

// ---- horizontal lifting step on sample quads (i .. i+3) of region rows ylo .. yhi -----------------------------
// CLAMP == false: the region's columns lie inside the picture; the neighbours come from 64/128-bit LDS reads.  A word
// that would fall off the half is replaced by the half's first / last word: it only feeds halo samples whose true
// neighbours lie outside the region, which no useful output depends on.
template < typename T, int F, int K, int RP, int RC, bool CLAMP >
__device__ __forceinline__ void
horizontal_step (T (*lds)[2 * RC], int tid, int ylo, int yhi, int hlo, int hhi)
{
  struct __attribute__ ((aligned (4 * sizeof (T)))) T4 { T v[4]; };
  constexpr Step st = filter_step (F, K);
  constexpr int NT = kind_ntaps (st.kind);
  constexpr int NQ = RC / 4;
  // neighbour window: samples i+off .. i+off+NT+2, fetched as aligned 4-sample words
  constexpr int FIRST = floor4 (st.off);
  constexpr int NW = (st.off + NT + 2 - FIRST) / 4 + 1;
  static_assert (RC % 4 == 0, "quads need 4-aligned halves");
#pragma unroll 2
  for (int it = tid; it < 2 * RP * NQ; it += kThreads) {
    const int q = it % NQ;
    const int y = it / NQ;
    const int i = 4 * q;
    if (y < ylo || y > yhi)
      continue;
    if (CLAMP && (i > hhi || i + 3 < hlo))
      continue;
    T *row = &lds[y][0];
    T *d = row + (st.target ? RC : 0);
    const T *o = row + (st.target ? 0 : RC);
    T s[NT + 3];
    if constexpr (CLAMP) {
#pragma unroll
      for (int t = 0; t < NT + 3; t++)
        s[t] = o[clampi (i + st.off + t, hlo, hhi)];
    } else {
      T4 w[NW];
#pragma unroll
      for (int m = 0; m < NW; m++)
        w[m] = reinterpret_cast < const T4 * >(o)[clampi (q + FIRST / 4 + m, 0, NQ - 1)];
#pragma unroll
      for (int t = 0; t < NT + 3; t++) {
        const int e = t + st.off - FIRST;
        s[t] = w[e >> 2].v[e & 3];
      }
    }
    T4 dv = *reinterpret_cast < const T4 * >(d + i);
#pragma unroll
    for (int k = 0; k < 4; k++)
      dv.v[k] = fwd_apply < T, F, K > (dv.v[k], s + k);
    *reinterpret_cast < T4 * >(d + i) = dv;
  }
}

// ---- where the last vertical step puts a row pair's four column quads: the level's sub-bands ---------------------
template < typename T > struct BandSink {
  char *ll, *hl, *lh, *hh;      // element (0,0) of each sub-band
  int ll_stride, hl_stride, lh_stride, hh_stride;       // bytes between sub-band rows
  int nc;                       // sub-band columns of the level
  bool vec;                     // band rows take 4-sample stores

  // (the row's parity is a constant of the step, the half a lane's: constant indices only, the tables stay in registers)
  template < int ODD > __device__ __forceinline__ void store (int half, int r, int c, const T * v) const
  {
    char *row;
    if constexpr (ODD != 0)
      row = half ? hh + (size_t) r * hh_stride : lh + (size_t) r * lh_stride;
    else
      row = half ? hl + (size_t) r * hl_stride : ll + (size_t) r * ll_stride;
    T *p = (T *) row + c;
    if (vec && c + 4 <= nc) {
      if constexpr (sizeof (T) == 2) {
        u32x2 pk;
        pk.x = (uint16_t) v[0] | ((uint32_t) (uint16_t) v[1] << 16);
        pk.y = (uint16_t) v[2] | ((uint32_t) (uint16_t) v[3] << 16);
        gstore < u32x2 > (p, pk);
      } else {
        gstore < u32x4 > (p, (u32x4) { (uint32_t) v[0], (uint32_t) v[1], (uint32_t) v[2], (uint32_t) v[3] });
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (c + k < nc)
          gstore < T > (p + k, v[k]);
    }
  }
};

// ---- vertical lifting step on the useful columns: 4 columns (one 64/128-bit LDS access) per item ------------------
// CLAMP == false: the region's rows lie inside the picture; only rows whose taps stay inside the region are computed
// (the skipped rows are halo no useful output depends on).
// LAST == true: the filter's final step, on the tile's useful row pairs only; the updated quad and its partner quad
// of the other row go to the sink (no LDS write-back, no separate output pass).
template < typename T, int F, int K, int RP, int RC, int H, int HC, bool CLAMP, bool LAST >
__device__ __forceinline__ void
vertical_step (T (*lds)[2 * RC], int tid, int vlo, int vhi, int r0, int cu0, const BandSink < T > &sink)
{
  struct __attribute__ ((aligned (4 * sizeof (T)))) T4 { T v[4]; };
  constexpr Step st = filter_step (F, K);
  constexpr int NT = kind_ntaps (st.kind);
  constexpr int IPH = (RC - 2 * HC) / 4;        // items per half row
  constexpr int IPR = 2 * IPH;
  constexpr int LO = LAST ? H : CLAMP ? 0 : cmax (0, -st.off);
  constexpr int HI = LAST ? RP - 1 - H : CLAMP ? RP - 1 : RP - 1 - cmax (0, st.off + NT - 1);
  constexpr int NR = HI - LO + 1;
  static_assert (!LAST || (-st.off >= 0 && -st.off <= NT - 1), "partner row outside the tap window");
#pragma unroll 2
  for (int it = tid; it < NR * IPR; it += kThreads) {
    const int cp = it % IPR;
    const int rp = LO + it / IPR;
    if (rp < vlo || rp > vhi)
      continue;
    const int half = cp >= IPH ? 1 : 0;
    const int ci = 4 * (cp - half * IPH);       // column inside the tile's useful columns
    const int col = half * RC + HC + ci;
    T4 tap[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const int rr = CLAMP ? clampi (rp + st.off + t, vlo, vhi) : rp + st.off + t;
      tap[t] = *reinterpret_cast < const T4 * >(&lds[2 * rr + 1 - st.target][col]);
    }
    T4 *dp = reinterpret_cast < T4 * >(&lds[2 * rp + st.target][col]);
    T4 d = *dp;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      T s[NT];
#pragma unroll
      for (int t = 0; t < NT; t++)
        s[t] = tap[t].v[e];
      d.v[e] = fwd_apply < T, F, K > (d.v[e], s);
    }
    if constexpr (!LAST) {
      *dp = d;
    } else {
      const int c = cu0 + ci;
      if (c < sink.nc) {
        sink.template store < st.target > (half, r0 + rp, c, d.v);
        sink.template store < 1 - st.target > (half, r0 + rp, c, tap[-st.off].v);
      }
    }
  }
}

// All lifting passes of one level on a staged region, synthesis steps N-1 .. 0: horizontal on every row of the region
// the picture has, then vertical on the useful columns, the last one feeding the sink.
// (r0, c0): sub-band row pair / column of the region origin.
template < typename T, int F, int RP, int RC, int H, int HC, bool HCLAMP >
__device__ __forceinline__ void
horizontal_steps (T (*lds)[2 * RC], int tid, int ylo, int yhi, int hlo, int hhi)
{
  constexpr int N = filter_nsteps (F);
  if constexpr (N == 4) {
    horizontal_step < T, F, 3, RP, RC, HCLAMP > (lds, tid, ylo, yhi, hlo, hhi);
    __syncthreads ();
    horizontal_step < T, F, 2, RP, RC, HCLAMP > (lds, tid, ylo, yhi, hlo, hhi);
    __syncthreads ();
  }
  horizontal_step < T, F, 1, RP, RC, HCLAMP > (lds, tid, ylo, yhi, hlo, hhi);
  __syncthreads ();
  horizontal_step < T, F, 0, RP, RC, HCLAMP > (lds, tid, ylo, yhi, hlo, hhi);
  __syncthreads ();
}

template < typename T, int F, int RP, int RC, int H, int HC, bool VCLAMP >
__device__ __forceinline__ void
vertical_steps (T (*lds)[2 * RC], int tid, int vlo, int vhi, int r0, int cu0, const BandSink < T > &sink)
{
  constexpr int N = filter_nsteps (F);
  if constexpr (N == 4) {
    vertical_step < T, F, 3, RP, RC, H, HC, VCLAMP, false > (lds, tid, vlo, vhi, r0, cu0, sink);
    __syncthreads ();
    vertical_step < T, F, 2, RP, RC, H, HC, VCLAMP, false > (lds, tid, vlo, vhi, r0, cu0, sink);
    __syncthreads ();
  }
  vertical_step < T, F, 1, RP, RC, H, HC, VCLAMP, false > (lds, tid, vlo, vhi, r0, cu0, sink);
  __syncthreads ();
  vertical_step < T, F, 0, RP, RC, H, HC, VCLAMP, true > (lds, tid, vlo, vhi, r0, cu0, sink);
}

// Everything behind the staging: the lifting passes of the staged region, the last one into the level's sub-bands.
template < typename T, int F, int RC >
__device__ __forceinline__ void
lift_region (T (*lds)[2 * RC], int tid, const IwtFwdJob & job, int r0, int c0, int vlo, int vhi, int hlo, int hhi, int nc)
{
  typedef FwdGeo < T, F > G;
  constexpr int RP = G::RP, H = G::H, HC = G::HC;
  static_assert (RC == G::RC, "the region of the filter's tile");
  if (hlo > 0 || hhi < RC - 1)  // the region sticks out of the picture: clamp columns
    horizontal_steps < T, F, RP, RC, H, HC, true > (lds, tid, 2 * vlo, 2 * vhi + 1, hlo, hhi);
  else
    horizontal_steps < T, F, RP, RC, H, HC, false > (lds, tid, 2 * vlo, 2 * vhi + 1, hlo, hhi);

  BandSink < T > sink;
  sink.ll = (char *) job.band[0];
  sink.hl = (char *) job.band[1];
  sink.lh = (char *) job.band[2];
  sink.hh = (char *) job.band[3];
  sink.ll_stride = job.band_stride[0];
  sink.hl_stride = job.band_stride[1];
  sink.lh_stride = job.band_stride[2];
  sink.hh_stride = job.band_stride[3];
  sink.nc = nc;
  sink.vec = (job.flags & 2) != 0;
  if (vlo > 0 || vhi < RP - 1)  // ... clamp rows
    vertical_steps < T, F, RP, RC, H, HC, true > (lds, tid, vlo, vhi, r0, c0 + HC, sink);
  else
    vertical_steps < T, F, RP, RC, H, HC, false > (lds, tid, vlo, vhi, r0, c0 + HC, sink);
}

}                               // namespace

template < typename T, int F >
__global__ __launch_bounds__ (kThreads)
void iwt_fwd_level_kernel (const IwtFwdJob * __restrict__ jobs, int njobs)
{
  typedef FwdGeo < T, F > G;
  constexpr int RP = G::RP, RC = G::RC, H = G::H, HC = G::HC, UR = G::UR, UC = G::UC;
  constexpr int NPS = rows_nps < T, RP, RC > ();
  constexpr int SH = filter_shift (F);
  __shared__ __attribute__ ((aligned (16))) T lds[2 * RP][2 * RC];

  const int tid = threadIdx.x;
  const int bid = xcd_tile_id (blockIdx.x, gridDim.x);
  const IwtFwdJob job = jobs[find_job (jobs, njobs, bid)];
  const int t = bid - job.tile_base;
  const int ty = mdiv (t, job.tiles_x, job.m_tiles_x);   // (the host's div_magic: no division by run-time geometry)
  const int tx = t - ty * job.tiles_x;
  const int nr = job.h >> 1, nc = job.w >> 1;
  const int r0 = ty * UR - H;  // sub-band row of region row pair 0
  const int c0 = tx * UC - HC;  // sub-band column of region column 0

  // region-local index ranges that exist in the picture
  const int vlo = max (0, -r0), vhi = min (RP - 1, nr - 1 - r0);
  const int hlo = max (0, -c0), hhi = min (RC - 1, nc - 1 - c0);

  // ---- stage the region's source rows in LDS, split into halves (and shifted) ------------------------------
  if (job.flags & 1) {
    // all loads are issued before the first LDS write
    uint2 v[NPS];
    rows_load < T, RP, RC, NPS > (v, job.src, job.src_stride, tid, r0, c0, nr, nc);
    rows_store < T, RP, RC, NPS, SH > (lds, v, tid);
  } else {
    typedef Ar < T > A;
    const char *base = (const char *) job.src;
    for (int it = tid; it < 2 * RP * RC; it += kThreads) {
      const int i = it % RC;
      const int y = it / RC;
      const int r = 2 * r0 + y, c = c0 + i;
      if (r >= 0 && r < 2 * nr && c >= 0 && c < nc) {
        const T *p = (const T *) (base + (size_t) r * job.src_stride) + 2 * c;
        T a = gload < T > (p), b = gload < T > (p + 1);
        if constexpr (SH != 0) {
          a = A::wrap (A::mul (a, 2));
          b = A::wrap (A::mul (b, 2));
        }
        lds[y][i] = a;
        lds[y][RC + i] = b;
      }
    }
  }
  __syncthreads ();

  lift_region < T, F, RC > (lds, tid, job, r0, c0, vlo, vhi, hlo, hhi, nc);
}

// The same level whose staging reads a PACKED picture (schro_hip_unpack_iwt_batch, level 0): a region sample's
// coordinate is clamped to the picture -- the edge extension of the encoder's converts (schroencoder.c:1053, 2454) --,
// its bits come out of the packed row's 16-byte words (unpack_fetch.h), the component is extracted and the format's
// offset removed in registers.  Everything behind the staging is the plane form's.
template < typename T, int F >
__global__ __launch_bounds__ (kThreads)
void iwt_fwd_packed_kernel (const IwtFwdPackedJob * __restrict__ jobs, int njobs)
{
  typedef FwdGeo < T, F > G;
  constexpr int RP = G::RP, RC = G::RC, H = G::H, HC = G::HC, UR = G::UR, UC = G::UC;
  constexpr int NPS = rows_nps < T, RP, RC > ();
  constexpr int SH = filter_shift (F);
  __shared__ __attribute__ ((aligned (16))) T lds[2 * RP][2 * RC];

  const int tid = threadIdx.x;
  const int bid = xcd_tile_id (blockIdx.x, gridDim.x);
  const IwtFwdPackedJob job = jobs[find_job (jobs, njobs, bid)];
  const int t = bid - job.tile_base;
  const int ty = mdiv (t, job.tiles_x, job.m_tiles_x);
  const int tx = t - ty * job.tiles_x;
  const int nr = job.h >> 1, nc = job.w >> 1;
  const int r0 = ty * UR - H;
  const int c0 = tx * UC - HC;
  const int vlo = max (0, -r0), vhi = min (RP - 1, nr - 1 - r0);
  const int hlo = max (0, -c0), hhi = min (RC - 1, nc - 1 - c0);

  // all loads are issued before the first LDS write
  uint2 v[NPS];
  rows_load_packed < T, RP, RC, NPS > (v, job, tid, r0, c0, nr, nc);
  rows_store < T, RP, RC, NPS, SH > (lds, v, tid);
  __syncthreads ();

  lift_region < T, F, RC > (lds, tid, job, r0, c0, vlo, vhi, hlo, hhi, nc);
}

namespace {

template < typename T, int F >
int
launch_one (hipStream_t stream, const IwtFwdJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH ((iwt_fwd_level_kernel < T, F >), dim3 (total_tiles), dim3 (kThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "forward iwt launch: %s", hipGetErrorString (e));
  return 0;
}

template < typename T >
int
launch_filter (hipStream_t stream, const IwtFwdJob * d_jobs, int njobs, int total_tiles, int filter)
{
  switch (filter) {
    case 0: return launch_one < T, 0 > (stream, d_jobs, njobs, total_tiles);
    case 1: return launch_one < T, 1 > (stream, d_jobs, njobs, total_tiles);
    case 2: return launch_one < T, 2 > (stream, d_jobs, njobs, total_tiles);
    case 3: return launch_one < T, 3 > (stream, d_jobs, njobs, total_tiles);
    case 4: return launch_one < T, 4 > (stream, d_jobs, njobs, total_tiles);
    case 5: return launch_one < T, 5 > (stream, d_jobs, njobs, total_tiles);
    case 6: return launch_one < T, 6 > (stream, d_jobs, njobs, total_tiles);
  }
  return set_error (SCHRO_HIP_EINVAL, "wavelet filter index %d out of range", filter);
}

template < typename T, int F >
int
launch_one_packed (hipStream_t stream, const IwtFwdPackedJob * d_jobs, int njobs, int total_tiles)
{
  SCHRO_LAUNCH ((iwt_fwd_packed_kernel < T, F >), dim3 (total_tiles), dim3 (kThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "forward iwt (packed) launch: %s", hipGetErrorString (e));
  return 0;
}

template < typename T >
int
launch_filter_packed (hipStream_t stream, const IwtFwdPackedJob * d_jobs, int njobs, int total_tiles, int filter)
{
  switch (filter) {
    case 0: return launch_one_packed < T, 0 > (stream, d_jobs, njobs, total_tiles);
    case 1: return launch_one_packed < T, 1 > (stream, d_jobs, njobs, total_tiles);
    case 2: return launch_one_packed < T, 2 > (stream, d_jobs, njobs, total_tiles);
    case 3: return launch_one_packed < T, 3 > (stream, d_jobs, njobs, total_tiles);
    case 4: return launch_one_packed < T, 4 > (stream, d_jobs, njobs, total_tiles);
    case 5: return launch_one_packed < T, 5 > (stream, d_jobs, njobs, total_tiles);
    case 6: return launch_one_packed < T, 6 > (stream, d_jobs, njobs, total_tiles);
  }
  return set_error (SCHRO_HIP_EINVAL, "wavelet filter index %d out of range", filter);
}

template < typename T >
void
geometry (int filter, int *uc, int *ur)
{
  switch (filter) {
    case 0: *uc = FwdGeo < T, 0 >::UC; *ur = FwdGeo < T, 0 >::UR; break;
    case 1: *uc = FwdGeo < T, 1 >::UC; *ur = FwdGeo < T, 1 >::UR; break;
    case 2: *uc = FwdGeo < T, 2 >::UC; *ur = FwdGeo < T, 2 >::UR; break;
    case 3: *uc = FwdGeo < T, 3 >::UC; *ur = FwdGeo < T, 3 >::UR; break;
    case 4: *uc = FwdGeo < T, 4 >::UC; *ur = FwdGeo < T, 4 >::UR; break;
    case 5: *uc = FwdGeo < T, 5 >::UC; *ur = FwdGeo < T, 5 >::UR; break;
    default: *uc = FwdGeo < T, 6 >::UC; *ur = FwdGeo < T, 6 >::UR; break;
  }
}

// the halo a tile's region has around its useful part: columns per half on either side, row pairs above and below
template < typename T >
void
halo (int filter, int *hc, int *hr)
{
  switch (filter) {
    case 0: *hc = FwdGeo < T, 0 >::HC; *hr = FwdGeo < T, 0 >::H; break;
    case 1: *hc = FwdGeo < T, 1 >::HC; *hr = FwdGeo < T, 1 >::H; break;
    case 2: *hc = FwdGeo < T, 2 >::HC; *hr = FwdGeo < T, 2 >::H; break;
    case 3: *hc = FwdGeo < T, 3 >::HC; *hr = FwdGeo < T, 3 >::H; break;
    case 4: *hc = FwdGeo < T, 4 >::HC; *hr = FwdGeo < T, 4 >::H; break;
    case 5: *hc = FwdGeo < T, 5 >::HC; *hr = FwdGeo < T, 5 >::H; break;
    default: *hc = FwdGeo < T, 6 >::HC; *hr = FwdGeo < T, 6 >::H; break;
  }
}

}                               // namespace

void
iwt_fwd_tile_geometry (int filter, int bpp, int *useful_cols, int *useful_row_pairs)
{
  if (bpp == 2)
    geometry < int16_t > (filter, useful_cols, useful_row_pairs);
  else
    geometry < int32_t > (filter, useful_cols, useful_row_pairs);
}

void
iwt_fwd_tile_halo (int filter, int bpp, int *halo_cols, int *halo_row_pairs)
{
  if (bpp == 2)
    halo < int16_t > (filter, halo_cols, halo_row_pairs);
  else
    halo < int32_t > (filter, halo_cols, halo_row_pairs);
}

int
launch_iwt_fwd_level (hipStream_t stream, const IwtFwdJob * d_jobs, int njobs, int total_tiles, int filter, int bpp)
{
  if (bpp == 2)
    return launch_filter < int16_t > (stream, d_jobs, njobs, total_tiles, filter);
  return launch_filter < int32_t > (stream, d_jobs, njobs, total_tiles, filter);
}

int
launch_iwt_fwd_packed (hipStream_t stream, const IwtFwdPackedJob * d_jobs, int njobs, int total_tiles, int filter, int bpp)
{
  if (bpp == 2)
    return launch_filter_packed < int16_t > (stream, d_jobs, njobs, total_tiles, filter);
  return launch_filter_packed < int32_t > (stream, d_jobs, njobs, total_tiles, filter);
}

}                               // namespace schro
