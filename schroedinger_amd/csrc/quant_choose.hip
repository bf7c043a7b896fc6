// quant_choose.hip -- the encoder's quantiser choice from the sub-band histograms (hist.hip), without a host step.
//
// What it computes: schro_encoder_calc_estimates (schroquantiser.c:688-732) -- per component, sub-band and quant index
// j < 60 an entropy estimate (schro_histogram_estimate_entropy, schrohistogram.c:266-343, times the arith context ratio)
// and an error estimate (schro_histogram_apply_table, :92-104) -- and then one of three engines over them:
// schro_encoder_lambda_to_entropy at a given frame lambda (:838-885), the same under schro_encoder_entropy_to_lambda's
// search for a bit count and once more at its answer (:738-756, :887-969), or schro_encoder_lambda_to_error under
// schro_encoder_error_to_lambda's search (:971-1119).  Doubles throughout, the reference's evaluation order, nothing
// fused (fp contract off): everything no transcendental touches is the host's bit for bit; the entropy estimates pass
// through exp (the noarith branch) or log (the other), each within 1 ulp on the device as on a host.
//
// qc_estimate_kernel: one wave per (picture, component, sub-band), lane j < 60 owns quant index j.  The 104 bins
// (counts * skip) go to LDS once, with their suffix sums.  get_range (start, 32000) is
//   (iexpx (i + 1) - start) / size * bins[i]  +  bins[i + 1] + ... + bins[103]  -  768 / 2048 * bins[103],  i = ilogx (start)
// summed left to right.  Every term is dyadic with at most 11 fractional bits (size <= 2048), and the bins of a sub-band
// sum to less than 2^32 counts * skip <= 2^10: every partial sum of the serial loop is exact in a double, so the suffix
// sum (exact too, in any order) plus the first term, minus the last, is the loop's value.  The error estimate is NOT of
// that kind -- 104 rounded products of a count and a weight -- and is the serial loop itself, in index order; the tables
// are stored [104][60], so the 60 lanes read neighbours at every step.
//
// qc_choose_kernel: one workgroup per picture runs the whole engine.  The picture's 2 x 57 x 60 estimates sit in LDS.  One
// evaluation: a wave per sub-band (four in turn) forms x = entropy + lambda * error, each of the two operations rounded,
// and reduces (x, j) to the serial scan's answer (schro_subband_pick_quant, :809-836: j = 0 unconditional, then strict <)
// -- the lowest j among the smallest x; a NaN at j > 0 never wins (it takes part as +inf behind every index), a NaN at
// j = 0 is never displaced --; then EVERY thread adds the chosen entries in (component, sub-band) order and walks the
// search's branches on its own: all hold the same doubles, so the control flow is uniform and `entropy_lo == entropy_hi`
// means what it means on a host.

#include "schro_hip_internal.h"
#include "dequant_one.h"

#pragma clang fp contract(off)

namespace schro {
namespace {

constexpr int kBins = SCHRO_HIP_HISTOGRAM_BINS, kCountWords = kBins + 1;
constexpr int kRanges = 12, kRangeEnd = 32000;
constexpr int kChooseThreads = 256, kChooseWaves = kChooseThreads / 64;
constexpr double kInvLog2 = 1.44269504088896338700;     // schroutils.c:306

// ilogx, iexpx, ilogx_size (schrohistogram.c:11-40) for 0 <= x < 32768 / 0 <= i <= 104
__device__ __forceinline__ int
qc_ilogx (int x)
{
  const int i = max (0, 28 - (int) __clz (x));
  return (x >> i) + 8 * i;
}

__device__ __forceinline__ int
qc_iexpx (int i)
{
  return i < 8 ? i : (8 | (i & 7)) << ((i >> 3) - 1);
}

__device__ __forceinline__ int
qc_size (int i)
{
  return i < 8 ? 1 : 1 << ((i >> 3) - 1);
}

// schro_histogram_get_range (hist, start, 32000); suffix[i] = bins[i] + ... + bins[103], suffix[104] = 0
__device__ __forceinline__ double
qc_range (const double *bins, const double *suffix, int start)
{
  if (start >= kRangeEnd)
    return 0.0;
  const int i = qc_ilogx (start);
  double x = (double) (qc_iexpx (i + 1) - start) / (double) qc_size (i) * bins[i];
  x += suffix[i + 1];
  x -= (double) (qc_iexpx (kBins) - kRangeEnd) / (double) qc_size (kBins - 1) * bins[kBins - 1];
  return x;
}

// schro_utils_entropy over schro_utils_probability_to_entropy (schroutils.c:308-327)
__device__ __forceinline__ double
qc_entropy (double a, double total)
{
  if (total == 0)
    return 0;
  const double x = a / total;
  if (x <= 0 || x >= 1.0)
    return 0 * total;
  return -(x * log (x) + (1 - x) * log (1 - x)) * kInvLog2 * total;
}

// schro_histogram_apply_table with table row j of a [104][60] table
__device__ __forceinline__ double
qc_apply (const double *bins, const double *__restrict__ table, int j)
{
  double sum = 0;
#pragma unroll 8
  for (int i = 0; i < kBins; i++)
    sum += bins[i] * table[i * kQcIndices + j];
  return sum;
}

__global__ __launch_bounds__ (64)
void qc_estimate_kernel (const QcPicture * __restrict__ pics, const double *__restrict__ tables, int have_bits, double *__restrict__ scratch)
{
  __shared__ double bins[kBins];
  __shared__ double suffix[kBins + 1];
  const int i = blockIdx.x, c = blockIdx.y, p = blockIdx.z, lane = threadIdx.x;
  const QcPicture & pic = pics[p];
  if (i >= 1 + 3 * pic.depth)
    return;
  const uint32_t *counts = pic.counts[c] + (size_t) i * kCountWords;
  const double skip = (double) pic.skip[i];
  for (int k = lane; k < kBins; k += 64)
    bins[k] = (double) counts[k] * skip;
  __syncthreads ();
  // (exact in any order: integers below 2^42)
  for (int k = lane; k <= kBins; k += 64) {
    double s = 0;
    for (int m = kBins - 1; m >= k; m--)
      s += bins[m];
    suffix[k] = s;
  }
  __syncthreads ();
  const int j = lane;
  if (j >= kQcIndices)
    return;
  const int factor = (int) kDevQuant.factor[j];  // schro_table_quant
  double bin[kRanges];
  bin[0] = qc_range (bins, suffix, 0);          // (the reference computes it here and again in its loop)
#pragma unroll
  for (int k = 0; k < kRanges; k++)
    bin[k] = qc_range (bins, suffix, (factor * ((1 << k) - 1) + 3) / 4);
  double est = 0;
  if (!pic.noarith) {
    est += bin[1];
    est += qc_entropy (bin[1], bin[0]);
    est += qc_entropy (bin[2], bin[1]);
    est += qc_entropy (bin[3], bin[2]);
    est += qc_entropy (bin[4], bin[3]);
    est += qc_entropy (bin[5], bin[4]);
    double post5 = 0;
#pragma unroll
    for (int k = 6; k < kRanges; k++)
      post5 += bin[k];
    est += qc_entropy (post5, post5 + bin[5]);
    // (have_bits: the plane layer refuses such a picture without the tables)
    const double ones = have_bits ? qc_apply (bins, tables + kQcTableDoubles, j) : 0.0;
    const double zeros = have_bits ? qc_apply (bins, tables + 2 * kQcTableDoubles, j) : 0.0;
    est += qc_entropy (ones, zeros + ones);
  } else {
    double x = bin[1] / bin[0];         // 0 / 0 = NaN when nothing was sampled into the bins
    x = 1.0 - exp (-0.5 * 25 * x);
    est += x * bin[0] + (1 - x) * bin[1];
    est += bin[1];
#pragma unroll
    for (int k = 1; k < kRanges; k++)
      est += 2 * bin[k];
  }
  est *= pic.ratio[c][i];
  const double err = qc_apply (bins, tables, j);
  const int at = (c * kQcBands + i) * kQcIndices + j;
  double *mine = scratch + (size_t) p * 2 * kQcEstimates;
  mine[at] = est;
  mine[kQcEstimates + at] = err;
  if (pic.est_entropy)
    pic.est_entropy[at] = est;
  if (pic.est_error)
    pic.est_error[at] = err;
}

struct QcChooseShared {
  double ent[kQcEstimates];
  double err[kQcEstimates];
  int idx[3 * kQcBands];
};

// schro_encoder_lambda_to_entropy / _to_error (on_error): called by every thread of the workgroup alike; leaves the
// chosen indices in sh.idx and returns the sum to every thread
__device__ double
qc_evaluate (QcChooseShared & sh, const QcPicture & pic, int nb, double frame_lambda, bool on_error, int &evaluations)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double inf = __builtin_huge_val ();
  for (int sb = wave; sb < 3 * nb; sb += kChooseWaves) {
    const int c = sb / nb, i = sb % nb;
    double lambda = frame_lambda;
    if (i == 0)
      lambda *= pic.scale[0];
    if (c > 0)
      lambda *= pic.scale[1];
    if (!on_error && i > 0 && (i - 1) % 3 == 2)         // SCHRO_SUBBAND_IS_DIAGONALLY_ORIENTED: not on the error path
      lambda *= pic.scale[2];
    const double weight = pic.weight[i];
    lambda /= weight * weight;
    double x = inf;
    if (lane < kQcIndices)
      x = sh.ent[sb * kQcIndices + lane] + lambda * sh.err[sb * kQcIndices + lane];
    const bool nan = x != x;
    const bool nan0 = __shfl ((int) nan, 0) != 0;
    if (nan)
      x = inf;
    int j = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ox = __shfl_xor (x, o);
      const int oj = __shfl_xor (j, o);
      if (ox < x || (ox == x && oj < j)) {
        x = ox;
        j = oj;
      }
    }
    if (lane == 0)
      sh.idx[sb] = nan0 ? 0 : j;
  }
  __syncthreads ();
  const double *from = on_error ? sh.err : sh.ent;
  double sum = 0;
  for (int sb = 0; sb < 3 * nb; sb++)
    sum += from[sb * kQcIndices + sh.idx[sb]];
  __syncthreads ();             // (the next evaluation writes idx)
  evaluations++;
  return sum;
}

__global__ __launch_bounds__ (kChooseThreads)
void qc_choose_kernel (const QcPicture * __restrict__ pics, const double *__restrict__ scratch)
{
  __shared__ QcChooseShared sh;
  const int tid = threadIdx.x;
  const QcPicture & pic = pics[blockIdx.x];
  const int nb = 1 + 3 * pic.depth;
  const double *mine = scratch + (size_t) blockIdx.x * 2 * kQcEstimates;
  // the picture's sub-bands, packed: component c, sub-band i at c * nb + i
  for (int t = tid; t < 3 * nb * kQcIndices; t += kChooseThreads) {
    const int sb = t / kQcIndices, j = t % kQcIndices;
    const int at = ((sb / nb) * kQcBands + sb % nb) * kQcIndices + j;
    sh.ent[t] = mine[at];
    sh.err[t] = mine[kQcEstimates + at];
  }
  __syncthreads ();

  int evaluations = 0, not_bracketed = 0;
  double frame_lambda, last;
  const double target = pic.target;
  if (pic.engine == SCHRO_HIP_QUANT_ENGINE_LAMBDA) {
    frame_lambda = target;
    last = qc_evaluate (sh, pic, nb, frame_lambda, false, evaluations);
  } else {
    // schro_encoder_entropy_to_lambda (:887-969) and schro_encoder_error_to_lambda (:1016-1098) are one text in two
    // senses: the entropy search starts from `hi` and steps up when hi < target, the error search starts from `lo` and
    // steps up when target < lo, and what "up" multiplies is the other end
    const bool on_error = pic.engine == SCHRO_HIP_QUANT_ENGINE_CONSTANT_ERROR;
    double lambda_hi, lambda_lo, v_hi, v_lo;
    if (!on_error) {
      lambda_hi = 1;
      v_hi = qc_evaluate (sh, pic, nb, lambda_hi, false, evaluations);
      if (v_hi < target) {
        v_lo = v_hi;
        lambda_lo = lambda_hi;
        for (int j = 0; j < 5; j++) {
          lambda_hi = lambda_lo * 100;
          v_hi = qc_evaluate (sh, pic, nb, lambda_hi, false, evaluations);
          if (v_hi > target)
            break;
          v_lo = v_hi;
          lambda_lo = lambda_hi;
        }
      } else {
        for (int j = 0; j < 5; j++) {
          lambda_lo = lambda_hi * 0.01;
          v_lo = qc_evaluate (sh, pic, nb, lambda_lo, false, evaluations);
          if (v_lo < target)
            break;
          v_hi = v_lo;
          lambda_hi = lambda_lo;
        }
      }
    } else {
      lambda_lo = 1;
      v_lo = qc_evaluate (sh, pic, nb, lambda_lo, true, evaluations);
      if (target < v_lo) {
        v_hi = v_lo;
        lambda_hi = lambda_lo;
        for (int j = 0; j < 5; j++) {
          lambda_lo = lambda_hi * 100;
          v_lo = qc_evaluate (sh, pic, nb, lambda_lo, true, evaluations);
          if (target > v_lo)
            break;
          v_hi = v_lo;
          lambda_hi = lambda_lo;
        }
      } else {
        for (int j = 0; j < 5; j++) {
          lambda_hi = lambda_lo * 0.01;
          v_hi = qc_evaluate (sh, pic, nb, lambda_hi, true, evaluations);
          if (target < v_hi)
            break;
          v_lo = v_hi;
          lambda_lo = lambda_hi;
        }
      }
    }
    if (v_lo == v_hi) {
      frame_lambda = __dsqrt_rn (lambda_lo * lambda_hi);
    } else {
      not_bracketed = v_lo > target || v_hi < target;
      const int halvings = on_error ? 14 : 7;
      for (int j = 0; j < halvings; j++) {
        if (v_hi == v_lo)
          break;
        const double lambda_mid = __dsqrt_rn (lambda_lo * lambda_hi);
        const double v_mid = qc_evaluate (sh, pic, nb, lambda_mid, on_error, evaluations);
        if (v_mid > target) {
          lambda_hi = lambda_mid;
          v_hi = v_mid;
        } else {
          lambda_lo = lambda_mid;
          v_lo = v_mid;
        }
      }
      frame_lambda = __dsqrt_rn (lambda_hi * lambda_lo);
    }
    if (!on_error)              // rdo_bit_allocation evaluates at its answer (:755); constant_error does not
      last = qc_evaluate (sh, pic, nb, frame_lambda, false, evaluations);
    else {
      // what its last evaluation returned: the chosen errors, added again in order
      last = 0;
      for (int sb = 0; sb < 3 * nb; sb++)
        last += sh.err[sb * kQcIndices + sh.idx[sb]];
    }
  }

  SchroHipQuantChoice *out = pic.result;
  if (tid < 3 * kQcBands) {
    const int c = tid / kQcBands, i = tid % kQcBands;
    const bool live = i < nb;
    const int q = live ? sh.idx[c * nb + i] : 0;
    out->quant_index[c][i] = q;
    out->chosen_entropy[c][i] = live ? sh.ent[(c * nb + i) * kQcIndices + q] : 0.0;
    out->chosen_error[c][i] = live ? sh.err[(c * nb + i) * kQcIndices + q] : 0.0;
  }
  if (tid == 0) {
    out->frame_lambda = frame_lambda;
    out->sum = last;
    out->evaluations = evaluations;
    out->not_bracketed = not_bracketed;
    out->reserved = 0;
  }
}

}                               // namespace

int
launch_quant_choose (hipStream_t stream, const QcPicture * d_pics, int npics, const double *tables, int have_bits, double *scratch)
{
  SCHRO_LAUNCH (qc_estimate_kernel, dim3 (kQcBands, 3, npics), dim3 (64), 0, stream, d_pics, tables, have_bits, scratch);
  SCHRO_LAUNCH (qc_choose_kernel, dim3 (npics), dim3 (kChooseThreads), 0, stream, d_pics, (const double *) scratch);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "quant choose launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
