// quant.hip -- the encoder's quantisation between the forward wavelet and the entropy coder.
//
// What it computes, per codeblock of a sub-band (schro_encoder_quantise_subband, schroencoder.c:3729-3785): the
// quantised value into the quant frame and, in the same pass, the dequantised value back into the coefficient frame --
// the reconstruction the encoder's local decode transforms (:2697-2700).  Bit for bit the reference's arithmetic:
//   s16 (schro_frame_data_quantise, :3485-3553): four 16-bit Orc programs by quant index (schroorc-dist.c:10746,
//     :10929, :11131) -- every step wraps at 16 bits (absw, shlw 2, subw, mullw), and the quotient comes from a shift
//     (multiples of 4), a 32-bit reciprocal multiply (index 3) or mulhuw by schro_table_inverse_quant (the rest), NOT
//     from schro_quantise's division;
//   s32: schro_quantise_s32 (schroutils.c:248-257), C int arithmetic, truncating division, |x| < 2^28;
//   the LL band of an intra picture: schro_frame_data_quantise_dc_predict (:3591-3667), one raster-order recurrence
//     over the band (a codeblock never reads its right neighbour) -- quantise_dc_kernel sweeps its anti-diagonals.
// One deliberate departure: the reference's s16 zero test (schro_frame_data_is_zero, :4043-4070) sums |q| per row in
// 16 bits and calls a row zero when that sum is a non-zero multiple of 65536 (its own FIXME); the summary written here
// is the true answer (nonzero == 0 exactly when every quantised sample is zero).
//
// quantise_kernel: one 256-thread workgroup = a 64 x 64 sample tile of one codeblock, 4 samples x 4 rows per lane -- the
// job and tile shape of dequant_kernel; all planes of a call in one launch, every per-codeblock constant in the job.
// Codeblocks start at any sample (xmin = width * x / horiz_codeblocks), so the 4-sample accesses are 8 / 16-byte
// accesses at 2 / 4-byte alignment; a codeblock's last columns go sample by sample.  Bound: HBM, 3 x bpp bytes per
// sample (coefficient read, quantised and reconstructed value written).  The summary: a wave reduction, the waves'
// results through LDS, then one add and one max per workgroup that has anything to report.

#include "schro_hip_internal.h"

namespace schro {
namespace {

constexpr int kQThreads = 256, kQTW = 64, kQRows = 4, kQTH = 16 * kQRows;
constexpr int kDcThreads = SCHRO_HIP_QUANTISE_DC_THREADS;

struct QuantTables4 {
  uint32_t factor[61], off12[61], off38[61], inverse[61];
};
constexpr QuantTables4
make_quant_tables4 ()
{
  QuantTables4 t = { };
  for (int q = 0; q <= 60; q++) {
    // Dirac specification 13.3.1, dequant.hip's closed forms (pinned there against the reference's numbers); here they are
    // held by the every-value, every-index test on the device, whose checker reads tests/golden/quant_tables_encoder.json
    const uint64_t base = (uint64_t) 1 << (q / 4);
    const uint64_t f = (q & 3) == 0 ? 4 * base : (q & 3) == 1 ? (503829 * base + 52958) / 105917
        : (q & 3) == 2 ? (665857 * base + 58854) / 117708 : (440253 * base + 32722) / 65444;
    t.factor[q] = (uint32_t) f;
    t.off12[q] = q == 0 ? 1u : q == 1 ? 2u : (uint32_t) ((f + 1) / 2);
    t.off38[q] = q == 0 ? 1u : (uint32_t) ((f * 3 + 4) / 8);
  }
  // schro_table_inverse_quant (schrotables.c:63-80) has no closed form that gives all 61 entries (it was rounded from
  // floating point): the numbers themselves, compared with that fixture on the CPU (tests/test_quantise_api.py); 0 where
  // the index is a multiple of 4 (the shift form)
  constexpr uint16_t inv[61] = { 0, 52429, 43691, 37449, 0, 52429, 47663, 40330, 0, 55188, 45590, 38836, 0, 55188, 46603, 38836,
    0, 55188, 46091, 38836, 0, 55188, 46346, 39017, 0, 55188, 46346, 38926, 0, 55098, 46346, 38971, 0, 55098, 46346, 38971,
    0, 55120, 46346, 38971, 0, 55109, 46338, 38966, 0, 55109, 46342, 38969, 0, 55109, 46342, 38969, 0, 55109, 46341, 38968,
    0, 55109, 46341, 38968, 0
  };
  for (int q = 0; q <= 60; q++)
    t.inverse[q] = inv[q];
  return t;
}
constexpr QuantTables4 kQuantTab = make_quant_tables4 ();
static __device__ const QuantTables4 kDevQuantTab = make_quant_tables4 ();      // (the resolve launch looks the quantiser up)

// form, factor, both offsets, shift and inverse of a codeblock, as schro_frame_data_quantise sets them up
// (schroencoder.c:3492-3504, :3543-3544); s32 and the DC band: schro_quantise's offset - factor / 2
__host__ __device__ __forceinline__ void
quant_constants (const QuantTables4 & tab, QuantJob * job, int quant_index, int is_intra, int bpp)
{
  const int q = quant_index < 0 ? 0 : (quant_index > 60 ? 60 : quant_index);
  job->factor = tab.factor[q];
  job->offset = is_intra ? tab.off12[q] : tab.off38[q];
  job->inverse = tab.inverse[q];
  job->shift = (q >> 2) + 2;
  if (bpp == 4) {
    job->form = kQuantDivide;
    job->qoff = (int32_t) job->offset - (int32_t) (job->factor / 2);
    return;
  }
  job->qoff = (int32_t) job->offset - (int32_t) (job->factor >> 1);
  if (q == 0) {
    job->form = kQuantCopy;
  } else if ((q & 3) == 0) {
    job->form = kQuantShift;
  } else if (q == 3) {
    job->form = kQuantRecip32;
    job->shift += 16;
  } else {
    job->form = kQuantRecip16;
    if (q > 8)
      job->qoff--;
  }
}

// schro_quantise / schro_dequantise (schroutils.c:179-235), C int arithmetic (wrapping where C's would overflow)
__device__ __forceinline__ int32_t
quantise_divide (int32_t v, uint32_t factor, uint32_t offset, int32_t qoff)
{
  if (v == 0)
    return 0;
  const uint32_t mag = v < 0 ? 0u - (uint32_t) v : (uint32_t) v;
  const int32_t x4 = (int32_t) (mag << 2);
  int32_t x = 0;
  if (x4 >= (int32_t) offset)
    x = (int32_t) ((uint32_t) x4 - (uint32_t) qoff) / (int32_t) factor;
  return v < 0 ? (int32_t) (0u - (uint32_t) x) : x;
}

__device__ __forceinline__ int32_t
dequantise_c (int32_t q, uint32_t factor, uint32_t offset)
{
  if (q == 0)
    return 0;
  const uint32_t mag = q < 0 ? 0u - (uint32_t) q : (uint32_t) q;
  const int32_t d = (int32_t) (mag * factor + offset + 2u) >> 2;
  return q < 0 ? (int32_t) (0u - (uint32_t) d) : d;
}

// one sample: q the quantised value, the return value the reconstruction
template < typename T >
__device__ __forceinline__ T
quantise_one (T xin, const QuantJob & job, T & q)
{
  if constexpr (sizeof (T) == 4) {
    q = quantise_divide (xin, job.factor, job.offset, job.qoff);
    return dequantise_c (q, job.factor, job.offset);
  } else {
    if (job.form == kQuantCopy) {
      q = xin;
      return xin;
    }
    const int32_t x = xin;
    const int32_t sign = x > 0 ? 1 : (x < 0 ? -1 : 0);          // signw
    const uint32_t a = (uint32_t) (x < 0 ? -x : x) & 0xffffu;   // absw: -32768 stays
    const uint32_t c = ((a << 2) - (uint32_t) job.qoff) & 0xffffu;      // shlw 2, subw -- as mulhuw / shruw see it
    uint32_t e;
    if (job.form == kQuantShift)
      e = c >> job.shift;                                       // shruw
    else if (job.form == kQuantRecip32)
      e = (c * job.inverse + 32768u) >> job.shift;              // muluwl, addl, shrul; convlw below
    else
      e = ((c * job.inverse) >> 16) >> job.shift;               // mulhuw, shruw
    const int32_t e16 = (int16_t) e;
    const int16_t qq = (int16_t) (e16 * sign);                  // mullw
    q = qq;
    const int32_t s2 = qq > 0 ? 1 : (qq < 0 ? -1 : 0);
    const int16_t f = (int16_t) (e16 * (int32_t) (int16_t) job.factor); // mullw by the factor as loadpw truncates it
    const int16_t g = (int16_t) (f + (int32_t) (int16_t) (job.offset + 2u));    // addw
    return (int16_t) ((g >> 2) * s2);                           // shrsw 2, mullw
  }
}

template < typename T >
__device__ __forceinline__ void
load4 (const T * p, int n, T * v)
{
  if (n == 4) {
    if constexpr (sizeof (T) == 2) {
      const u32x2 a = gload < u32x2_u > (p);
      v[0] = (T) a.x;
      v[1] = (T) (a.x >> 16);
      v[2] = (T) a.y;
      v[3] = (T) (a.y >> 16);
    } else {
      const u32x4 a = gload < u32x4_u > (p);
      v[0] = (T) a.x;
      v[1] = (T) a.y;
      v[2] = (T) a.z;
      v[3] = (T) a.w;
    }
  } else {
    for (int e = 0; e < 4; e++)
      v[e] = e < n ? gload < T > (p + e) : (T) 0;
  }
}

template < typename T >
__device__ __forceinline__ void
store4 (T * p, int n, const T * v)
{
  if (n == 4) {
    if constexpr (sizeof (T) == 2) {
      u32x2 o;
      o.x = (uint32_t) (uint16_t) v[0] | ((uint32_t) (uint16_t) v[1] << 16);
      o.y = (uint32_t) (uint16_t) v[2] | ((uint32_t) (uint16_t) v[3] << 16);
      gstore < u32x2_u > (p, o);
    } else {
      gstore < u32x4_u > (p, (u32x4) { (uint32_t) v[0], (uint32_t) v[1], (uint32_t) v[2], (uint32_t) v[3] });
    }
  } else {
    for (int e = 0; e < n; e++)
      gstore < T > (p + e, v[e]);
  }
}

// the summary's two words: plain vector atomics on global memory, device scope
__device__ __forceinline__ void
summary_add (SchroHipCodeblockSummary * s, uint32_t cnt, uint32_t mx)
{
  __hip_atomic_fetch_add ((SCHRO_GLOBAL uint32_t *) &s->nonzero, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max ((SCHRO_GLOBAL uint32_t *) &s->max_abs, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t
abs_u32 (int32_t q)
{
  return q < 0 ? 0u - (uint32_t) q : (uint32_t) q;
}

// a codeblock's summary from what the lanes of this workgroup found: a wave reduction, the four waves' results through
// LDS, then one add and one max for the workgroup -- if it has anything to report (all workgroups of a codeblock meet on
// the same two words: an atomic pair per wave measured 1.9 x slower on bands that are one codeblock, profiles/r13_quantise.txt)
__device__ __forceinline__ void
summary_report (SchroHipCodeblockSummary * s, uint32_t cnt, uint32_t mx)
{
  __shared__ uint32_t wave_cnt[kQThreads / 64], wave_mx[kQThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += (uint32_t) __shfl_xor ((int) cnt, o);
    mx = max (mx, (uint32_t) __shfl_xor ((int) mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    wave_cnt[threadIdx.x >> 6] = cnt;
    wave_mx[threadIdx.x >> 6] = mx;
  }
  __syncthreads ();
  if (threadIdx.x == 0) {
    cnt = mx = 0;
#pragma unroll
    for (int k = 0; k < kQThreads / 64; k++) {
      cnt += wave_cnt[k];
      mx = max (mx, wave_mx[k]);
    }
    if (cnt)
      summary_add (s, cnt, mx);
  }
}

template < typename T >
__global__ __launch_bounds__ (kQThreads)
void quantise_kernel (const QuantJob * __restrict__ jobs, int njobs)
{
  const int bid = blockIdx.x;
  const QuantJob job = jobs[find_dequant_job (jobs, njobs, bid)];
  const int t = bid - job.tile_base;
  const int ty = t / job.tiles_x, tx = t - ty * job.tiles_x;
  const int x = tx * kQTW + 4 * (threadIdx.x & 15), y0 = ty * kQTH + (threadIdx.x >> 4);
  // (no lane leaves early: the summary's reduction runs over the whole wave)
  const int n = x < job.w ? min (4, job.w - x) : 0;
  // a lane's rows lie 16 apart; the coefficients of all of them are asked for before the first is used
  T v[kQRows][4];
#pragma unroll
  for (int r = 0; r < kQRows; r++) {
    const int y = y0 + 16 * r;
    v[r][0] = v[r][1] = v[r][2] = v[r][3] = 0;
    if (n && y < job.h)
      load4 < T > ((const T *) ((const char *) job.coeffs + (size_t) y * job.stride) + x, n, v[r]);
  }
  uint32_t cnt = 0, mx = 0;
#pragma unroll
  for (int r = 0; r < kQRows; r++) {
    const int y = y0 + 16 * r;
    if (!n || y >= job.h)
      continue;
    T q[4], rec[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      rec[e] = quantise_one < T > (v[r][e], job, q[e]);
      if (e < n) {
        cnt += q[e] != 0;
        mx = max (mx, abs_u32 (q[e]));
      }
    }
    const size_t off = (size_t) y * job.stride;
    store4 < T > ((T *) ((char *) job.quant + off) + x, n, q);
    if (job.form != kQuantCopy)
      store4 < T > ((T *) ((char *) job.coeffs + off) + x, n, rec);
  }
  summary_report (job.summary, cnt, mx);
}

// The intra LL band.  Sample (j, i) -- row j, column i -- needs the RECONSTRUCTED (j, i - 1), (j - 1, i) and
// (j - 1, i - 1): all samples of an anti-diagonal d = i + j are independent.  One workgroup per band walks the
// diagonals; the reconstructions of the two previous ones stay in LDS, indexed by row (three buffers in turn, one
// workgroup barrier per diagonal); a diagonal longer than the workgroup is walked in strides.  Nothing is handed from
// one workgroup to another.  A band is a few hundred diagonals and the bands of a call run side by side: the kernel is
// bounded by the barrier and the LDS round trip of a step, not by bytes.
template < typename T >
__global__ __launch_bounds__ (kDcThreads)
void quantise_dc_kernel (const QuantDcJob * __restrict__ jobs, const QuantDcRec * __restrict__ recs, int lds_rows)
{
  extern __shared__ __attribute__ ((aligned (16))) int32_t dc_lds[];
  const QuantDcJob job = jobs[blockIdx.x];
  const int w = job.w, h = job.h, tid = threadIdx.x;
  recs += job.rec_base;
  int32_t *cur = dc_lds, *p1 = dc_lds + lds_rows, *p2 = dc_lds + 2 * lds_rows;
  int k = 0;                    // the codeblock of this lane's last sample, and what the lane has found there so far
  QuantDcRec rec = recs[0];
  uint32_t cnt = 0, mx = 0;
  auto at = [&] (void *base, int j, int i)->T * {
    return (T *) ((char *) base + (size_t) j * job.stride) + i;
  };
  // the coefficient of this lane's first sample on the next diagonal is asked for a step ahead
  T ahead = tid == 0 ? gload < T > (at (job.coeffs, 0, 0)) : (T) 0;
  for (int d = 0; d < w + h - 1; d++) {
    const int jlo = max (0, d - w + 1), jhi = min (h - 1, d);
    const T first = ahead;
    {
      const int nlo = max (0, d + 1 - w + 1), nhi = min (h - 1, d + 1), j = nlo + tid;
      if (d + 1 < w + h - 1 && j <= nhi)
        ahead = gload < T > (at (job.coeffs, j, d + 1 - j));
    }
    for (int j = jlo + tid; j <= jhi; j += kDcThreads) {
      const int i = d - j;
      const int32_t x = j == jlo + tid ? first : gload < T > (at (job.coeffs, j, i));
      int32_t pred;
      if (j > 0) {
        if (i > 0) {
          const int32_t a = p1[j] + p1[j - 1] + p2[j - 1] + 1;
          if constexpr (sizeof (T) == 2)
            pred = (a * 21845 + 10922) >> 16;   // schro_divide3
          else
            pred = a < 0 ? (a - 2) / 3 : a / 3; // schro_divide (a, 3)
        } else {
          pred = p1[j - 1];
        }
      } else {
        pred = i > 0 ? p1[j] : 0;
      }
      if (i < rec.x0 || i >= rec.x1 || j < rec.y0 || j >= rec.y1) {
        if (cnt)
          summary_add (job.summary + rec.index, cnt, mx);
        cnt = mx = 0;
        for (k = 0; k < job.nrec - 1; k++) {
          rec = recs[k];
          if (i >= rec.x0 && i < rec.x1 && j >= rec.y0 && j < rec.y1)
            break;
        }
        rec = recs[k];
      }
      const int32_t qoff = (int32_t) rec.offset - (int32_t) (rec.factor >> 1);
      const int32_t q = quantise_divide ((int32_t) ((uint32_t) x - (uint32_t) pred), rec.factor, rec.offset, qoff);
      const T out = (T) (int32_t) ((uint32_t) dequantise_c (q, rec.factor, rec.offset) + (uint32_t) pred);
      const T qs = (T) q;       // (the s16 stores truncate)
      gstore < T > (at (job.quant, j, i), qs);
      gstore < T > (at (job.coeffs, j, i), out);
      cur[j] = out;
      cnt += qs != 0;
      mx = max (mx, abs_u32 (qs));
    }
    __syncthreads ();
    int32_t *const t = p2;
    p2 = p1;
    p1 = cur;
    cur = t;
  }
  if (cnt)
    summary_add (job.summary + rec.index, cnt, mx);
}

// schro_hip_quantise_chosen_batch: the constants the host would have put into the records, from quant indices that are
// on the device.  A record's `pad` holds its sub-band; the run it lies in names its plane's row of chosen indices.  A value
// outside 0 .. 60 is clamped into range and counted.
__device__ __forceinline__ int
chosen_index (const QuantChosen * __restrict__ runs, int nruns, int t, int subband, uint32_t * clamped, int *is_intra)
{
  int r = 0;
  while (r + 1 < nruns && t >= runs[r].first + runs[r].count)
    r++;
  *is_intra = runs[r].is_intra;
  const int32_t q = runs[r].chosen[subband];
  if (q < 0 || q > 60)
    __hip_atomic_fetch_add (clamped, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return q < 0 ? 0 : (q > 60 ? 60 : q);
}

__global__ __launch_bounds__ (256)
void quantise_resolve_kernel (QuantJob * __restrict__ jobs, int njobs, int first, const QuantChosen * __restrict__ runs, int nruns, int bpp,
    uint32_t * clamped)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= njobs)
    return;
  int is_intra;
  const int q = chosen_index (runs, nruns, first + t, jobs[t].pad, clamped, &is_intra);
  quant_constants (kDevQuantTab, jobs + t, q, is_intra, bpp);
}

__global__ __launch_bounds__ (256)
void quantise_resolve_dc_kernel (QuantDcRec * __restrict__ recs, int nrecs, const QuantChosen * __restrict__ runs, int nruns, uint32_t * clamped)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nrecs)
    return;
  int is_intra;
  const int q = chosen_index (runs, nruns, t, recs[t].pad, clamped, &is_intra);
  QuantJob j;
  quant_constants (kDevQuantTab, &j, q, is_intra, 4);   // (C schro_quantise at both depths)
  recs[t].factor = j.factor;
  recs[t].offset = j.offset;
}

}                               // namespace

int
launch_quantise_resolve (hipStream_t stream, QuantJob * d_jobs, int njobs, int first, const QuantChosen * d_runs, int nruns, int bpp,
    uint32_t * clamped)
{
  SCHRO_LAUNCH (quantise_resolve_kernel, dim3 (div_up (njobs, 256)), dim3 (256), 0, stream, d_jobs, njobs, first, d_runs, nruns, bpp, clamped);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "quantise resolve launch: %s", hipGetErrorString (e));
  return 0;
}

int
launch_quantise_resolve_dc (hipStream_t stream, QuantDcRec * d_recs, int nrecs, const QuantChosen * d_runs, int nruns, uint32_t * clamped)
{
  SCHRO_LAUNCH (quantise_resolve_dc_kernel, dim3 (div_up (nrecs, 256)), dim3 (256), 0, stream, d_recs, nrecs, d_runs, nruns, clamped);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "quantise resolve (DC) launch: %s", hipGetErrorString (e));
  return 0;
}

void
quant_tile_geometry (int *tw, int *th)
{
  *tw = kQTW;
  *th = kQTH;
}

void
quant_job_constants (QuantJob * job, int quant_index, int is_intra, int bpp)
{
  quant_constants (kQuantTab, job, quant_index, is_intra, bpp);
}

int
launch_quantise (hipStream_t stream, const QuantJob * d_jobs, int njobs, int total_tiles, int bpp)
{
  if (bpp == 2)
    SCHRO_LAUNCH ((quantise_kernel < int16_t >), dim3 (total_tiles), dim3 (kQThreads), 0, stream, d_jobs, njobs);
  else
    SCHRO_LAUNCH ((quantise_kernel < int32_t >), dim3 (total_tiles), dim3 (kQThreads), 0, stream, d_jobs, njobs);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "quantise launch: %s", hipGetErrorString (e));
  return 0;
}

int
launch_quantise_dc (hipStream_t stream, const QuantDcJob * d_jobs, int njobs, const QuantDcRec * d_recs, int max_rows, int bpp)
{
  const int lds_rows = (max_rows + 3) & ~3;
  const size_t lds = 3 * (size_t) lds_rows * sizeof (int32_t);
  if (bpp == 2)
    SCHRO_LAUNCH ((quantise_dc_kernel < int16_t >), dim3 (njobs), dim3 (kDcThreads), lds, stream, d_jobs, d_recs, lds_rows);
  else
    SCHRO_LAUNCH ((quantise_dc_kernel < int32_t >), dim3 (njobs), dim3 (kDcThreads), lds, stream, d_jobs, d_recs, lds_rows);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "quantise (DC) launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
