// lowdelay_enc.hip -- VC-2 low-delay slices written on the device: the twin of
// schro_encoder_encode_lowdelay_transform_data (schrolowdelay.c:764-1200).
//
// Per slice the reference searches the base quantiser index at which the slice fits its bytes
// (schro_encoder_pick_slice_index, :1116-1148), each probe a full quantisation + bit count of the slice
// (schro_encoder_estimate_slice, :927-1062), then writes it (schro_encoder_encode_slice, :785-839).  The only thing one
// slice needs from another is the RECONSTRUCTED LL band: its DC prediction (quantise_dc_block, :874-904) reads the left,
// upper and upper-left neighbours as the slices before it left them at their final index.  So the work is cut in three
// launches, each over all pictures of a call:
//
//   ldenc_estimate_kernel   one wave per slice, no dependency: for every base index 0 .. 64 the bits of the HIGH bands
//                           (sub-bands 1 .. 3 depth) up to their last non-zero value, luma and chroma apart -- 0 means "all
//                           zero".  Lane q owns quantiser index q (0 .. 60) and walks every sample of a band (broadcast
//                           from LDS): the length of a code needs no division -- with y = 4 |x| - off + factor the
//                           quantised value + 1 is y / factor, its bit length the largest k with factor << k <= y, one
//                           leading-zero count and one compare.  Lane b then gathers, band by band, the sums of index
//                           CLAMP (b - quant_matrix[i], 0, 60) from the lane that owns it.
//   ldenc_choose_kernel     the serial part, one workgroup per picture, a thread per slice, anti-diagonals of slices with a
//                           barrier between them: the reference's probes (index 0; 32, 16 .. 1 upwards; the final one),
//                           each the LL recurrence of the three components on samples kept in LDS plus two words of the
//                           table.  Leaves the base index of every slice and the reconstructed LL bands.
//   ldenc_pack_kernel       one wave per slice, no dependency: quantise at the chosen index (the LL prediction now reads
//                           final neighbours), exp-Golomb codes, prefix sum of their lengths inside the wave, bits OR-ed
//                           into a window of LDS words, whole words stored (bytes at the two ends of a slice, which it
//                           shares with its neighbours), 1-bits up to the slice's end.  A slice whose bits do not fit --
//                           the reference asserts -- is cut at its last bit and counted.
//
// quant_data is int16_t in the reference: an LL difference at index 0 reaches +-65535 and wraps when stored; estimate,
// dequantisation and bits all use the wrapped value, and so does this file (w16).  High-band values never wrap.

#include "schro_hip_internal.h"

#include <algorithm>

namespace schro {
namespace {

// schro_table_quant / schro_table_offset_1_2 by the generating formula (as lowdelay.hip; tests pin all 61 entries)
struct EncQuantTables {
  uint32_t factor[61], offset[61];
};
constexpr EncQuantTables
make_enc_quant_tables ()
{
  EncQuantTables t = { };
  for (int q = 0; q <= 60; q++) {
    const uint64_t base = (uint64_t) 1 << (q / 4);
    const uint64_t f = (q & 3) == 0 ? 4 * base : (q & 3) == 1 ? (503829 * base + 52958) / 105917
        : (q & 3) == 2 ? (665857 * base + 58854) / 117708 : (440253 * base + 32722) / 65444;
    t.factor[q] = (uint32_t) f;
    t.offset[q] = q == 0 ? 1u : q == 1 ? 2u : (uint32_t) ((f + 1) / 2);
  }
  return t;
}
static __device__ const EncQuantTables kEncQuant = make_enc_quant_tables ();

constexpr int kEstChunk = 256;  // band positions staged in LDS at a time (estimate)
constexpr int kWinWords = 68;   // pack: 64 codes of up to 32 bits behind up to 31 carried bits, and one word of slack

__device__ __forceinline__ int32_t
w16 (int32_t v)
{
  return (int32_t) (int16_t) v;
}

// schro_quantise (schroutils.c:197-229) for |value| < 2^17
__device__ __forceinline__ int32_t
enc_quantise (int32_t value, uint32_t factor, uint32_t offset)
{
  const uint32_t x = (value < 0 ? 0u - (uint32_t) value : (uint32_t) value) << 2;
  if (value == 0 || x < offset)
    return 0;
  const uint32_t q = (x - offset + factor / 2u) / factor;
  return value < 0 ? -(int32_t) q : (int32_t) q;
}

// schro_dequantise (:179-189)
__device__ __forceinline__ int32_t
enc_dequantise (int32_t q, uint32_t factor, uint32_t offset)
{
  if (q == 0)
    return 0;
  const uint32_t mag = q < 0 ? 0u - (uint32_t) q : (uint32_t) q;
  const int32_t r = (int32_t) (mag * factor + offset + 2u) >> 2;
  return q < 0 ? -r : r;
}

// schro_pack_estimate_sint (schropack.c:214-226) of an int16 value
__device__ __forceinline__ int
sint_bits (int32_t q)
{
  const uint32_t mag = q < 0 ? 0u - (uint32_t) q : (uint32_t) q;
  const int l = 32 - __clz ((int) (mag + 1u));
  return 2 * l - 1 + (mag ? 1 : 0);
}

// schro_pack_encode_sint (:163-178): the code right-aligned, its length 1 .. 32
__device__ __forceinline__ uint32_t
sint_code (int32_t q, int *len)
{
  const uint32_t mag = q < 0 ? 0u - (uint32_t) q : (uint32_t) q;
  if (mag == 0) {
    *len = 1;
    return 1u;
  }
  const uint32_t v = mag + 1u;
  const int l = 32 - __clz ((int) v);
  uint32_t d = v & ((1u << (l - 1)) - 1u);      // the l - 1 bits under the leading one, each sent as "0 b"
  d = (d | (d << 8)) & 0x00ff00ffu;
  d = (d | (d << 4)) & 0x0f0f0f0fu;
  d = (d | (d << 2)) & 0x33333333u;
  d = (d | (d << 1)) & 0x55555555u;
  *len = 2 * l;
  return (d << 2) | 2u | (q < 0 ? 1u : 0u);
}

__device__ __forceinline__ int
enc_ilog2up (uint32_t x)
{                               // schrolowdelay.c:94-105: the bit length
  return x ? 32 - __clz ((int) x) : 0;
}

// sub-band `index` of a component and the slice's rectangle in it (schro_subband_get_frame_data, schroparams.c:319-352;
// schro_frame_data_get_codeblock, schroframe.c:1865-1884): `first` is the rectangle's first sample, `pitch` the bytes
// between its rows
struct EncRect {
  const uint8_t *first;
  size_t pitch;
  int xmin, ymin, bw, bh;
};
__device__ __forceinline__ EncRect
enc_rect (const void *plane, int stride, int iwt_w, int iwt_h, int depth, int index, int sx, int sy, int nh, int nv)
{
  const int position = index == 0 ? 0 : ((index - 1) / 3 + 1) * 4 - 3 + (index - 1) % 3;
  const int shift = depth - (position >> 2);
  const int w = iwt_w >> shift, h = iwt_h >> shift;
  EncRect r;
  r.xmin = (w * sx) / nh;
  r.ymin = (h * sy) / nv;
  r.bw = (w * (sx + 1)) / nh - r.xmin;
  r.bh = (h * (sy + 1)) / nv - r.ymin;
  r.pitch = (size_t) stride << shift;
  r.first = (const uint8_t *) plane + ((position & 2) ? r.pitch >> 1 : 0) + ((position & 1) ? (size_t) w * 2 : 0)
      + (size_t) r.ymin * r.pitch + (size_t) r.xmin * 2;
  return r;
}

__device__ __forceinline__ int32_t
enc_sample (const EncRect & r, int x, int y)
{
  return gload < int16_t > ((const int16_t *) (r.first + (size_t) y * r.pitch) + x);
}

__device__ __forceinline__ void
enc_slice_bytes (const SliceParams & P, int s, uint32_t * offset, uint32_t * bytes)
{
  // slice s: s whole slices plus one extra byte per wrap of the accumulator (:1171-1190)
  const uint32_t wraps = (uint32_t) (((uint64_t) s * (uint32_t) P.remainder) / (uint32_t) P.denom);
  const uint32_t wraps1 = (uint32_t) (((uint64_t) (s + 1) * (uint32_t) P.remainder) / (uint32_t) P.denom);
  *offset = (uint32_t) s * (uint32_t) P.n_bytes + wraps;
  *bytes = (uint32_t) P.n_bytes + (wraps1 - wraps);
}

// ---- estimate ---------------------------------------------------------------------------------------------------------

// one sample against the lane's quantiser: the bits of its code, and whether it is non-zero
__device__ __forceinline__ uint32_t
est_bits (uint32_t x4, uint32_t factor, uint32_t foff, int clzf, bool * nz)
{
  // quantised + 1 = y / factor with y = max (4 |x| - off, 0) + factor (the dead zone lies inside the first factor);
  // k = its bit length - 1: factor << (clz (factor) - clz (y)) has y's bit length, one compare says which side
  const uint32_t y = max (x4 + foff, factor);
  const int k0 = clzf - __clz ((int) y);
  const int k = k0 - (int) ((factor << k0) > y);
  *nz = k != 0;
  return k ? 2u * (uint32_t) k + 2u : 1u;
}

__global__ __launch_bounds__ (64)
void ldenc_estimate_kernel (const EncJob * __restrict__ jobs, const SliceParams P)
{
  __shared__ uint32_t x4s[2][kEstChunk];
  const EncJob job = jobs[blockIdx.y];
  const int lane = (int) threadIdx.x;
  const int s = (int) blockIdx.x;
  const int sy = s / P.nh, sx = s - sy * P.nh;
  const int qi = min (lane, 60);
  const uint32_t factor = kEncQuant.factor[qi];
  const uint32_t foff = factor - (kEncQuant.offset[qi] - factor / 2u);  // (offset - factor / 2 is -1 at index 0)
  const int clzf = __clz ((int) factor);
  const int nsub = 1 + 3 * P.depth;
  uint32_t *out = job.est + (size_t) s * 130;
#pragma unroll 1
  for (int k = 0; k < 2; k++) {
    const int iwt_w = k ? P.iwt_cw : P.iwt_lw, iwt_h = k ? P.iwt_ch : P.iwt_lh;
    const void *pa = k ? job.comp[1] : job.comp[0];
    const int stride_a = k ? job.stride[1] : job.stride[0];
    uint32_t acc1 = 0, net1 = 0, acc2 = 0, net2 = 0;    // base index `lane`, and 64
#pragma unroll 1
    for (int i = 1; i < nsub; i++) {
      const EncRect ra = enc_rect (pa, stride_a, iwt_w, iwt_h, P.depth, i, sx, sy, P.nh, P.nv);
      const EncRect rb = enc_rect (job.comp[2], job.stride[2], iwt_w, iwt_h, P.depth, i, sx, sy, P.nh, P.nv);
      const int n = ra.bw * ra.bh;
      uint32_t total = 0, upto = 0;     // the band at the lane's quantiser: all its bits; those up to the last non-zero
#pragma unroll 1
      for (int c0 = 0; c0 < n; c0 += kEstChunk) {
        const int cnt = min (kEstChunk, n - c0);
        for (int e = lane; e < cnt; e += 64) {
          const int idx = c0 + e, y = idx / ra.bw, x = idx - y * ra.bw;
          const int32_t va = enc_sample (ra, x, y);
          x4s[0][e] = (uint32_t) (va < 0 ? -va : va) << 2;
          if (k) {
            const int32_t vb = enc_sample (rb, x, y);
            x4s[1][e] = (uint32_t) (vb < 0 ? -vb : vb) << 2;
          }
        }
        __syncthreads ();
        if (k) {                // U and V value by value; trailing zeros count in pairs (:1052-1058)
          for (int e = 0; e < cnt; e++) {
            bool nza, nzb;
            total += est_bits (x4s[0][e], factor, foff, clzf, &nza);
            total += est_bits (x4s[1][e], factor, foff, clzf, &nzb);
            upto = (nza || nzb) ? total : upto;
          }
        } else {
          for (int e = 0; e < cnt; e++) {
            bool nz;
            total += est_bits (x4s[0][e], factor, foff, clzf, &nz);
            upto = nz ? total : upto;
          }
        }
        __syncthreads ();
      }
      // base index b takes this band at CLAMP (b - quant_matrix[i], 0, 60) (:965)
      const int q1 = min (max (lane - P.quant_matrix[i], 0), 60), q2 = min (max (64 - P.quant_matrix[i], 0), 60);
      const uint32_t t1 = (uint32_t) __shfl ((int) total, q1), u1 = (uint32_t) __shfl ((int) upto, q1);
      const uint32_t t2 = (uint32_t) __shfl ((int) total, q2), u2 = (uint32_t) __shfl ((int) upto, q2);
      net1 = u1 ? acc1 + u1 : net1;
      acc1 += t1;
      net2 = u2 ? acc2 + u2 : net2;
      acc2 += t2;
    }
    gstore < uint32_t > (out + 2 * lane + k, net1);
    if (lane == 0)
      gstore < uint32_t > (out + 2 * 64 + k, net2);
  }
}

// ---- choose -----------------------------------------------------------------------------------------------------------

// the prediction of LL sample (X, Y) from its reconstructed neighbours (schro_dc_predict, :765-783)
__device__ __forceinline__ int32_t
dc_pred (int X, int Y, int32_t left, int32_t up, int32_t upleft)
{
  if (Y > 0)
    return X > 0 ? ((left + up + upleft + 1) * 21845 + 10922) >> 16 : up;     // schro_divide3
  return X > 0 ? left : 0;
}

__global__ __launch_bounds__ (1024)
void ldenc_choose_kernel (const EncJob * __restrict__ jobs, const SliceParams P, const EncChooseLayout L)
{
  extern __shared__ int16_t choose_lds[];
  const EncJob & job = jobs[blockIdx.x];      // (members are read where they are used: a copy costs 16 SGPRs for the whole kernel)
  const int tid = (int) threadIdx.x, T = (int) blockDim.x;
  // a thread's samples: LDS where they fit, the call's scratch where not; element k of thread t at k * T + t
  int16_t *const buf = L.in_lds ? choose_lds : job.work;
  const int llw[2] = { P.iwt_lw >> P.depth, P.iwt_cw >> P.depth }, llh[2] = { P.iwt_lh >> P.depth, P.iwt_ch >> P.depth };
  const int q0 = P.quant_matrix[0];
  const int ndiag = P.nh + P.nv - 1;
#pragma unroll 1
  for (int d = 0; d < ndiag; d++) {
    const int sy_lo = max (0, d - (P.nh - 1)), cnt = min (P.nv - 1, d) - sy_lo + 1;
#pragma unroll 1
    for (int t0 = 0; t0 < cnt; t0 += T) {
      if (t0 + tid >= cnt)
        continue;
      const int sy = sy_lo + t0 + tid, sx = d - sy, s = sy * P.nh + sx;
      uint32_t offset, slice_bytes;
      enc_slice_bytes (P, s, &offset, &slice_bytes);
      const uint32_t budget = 8u * slice_bytes;
      const uint32_t header = 7u + (uint32_t) enc_ilog2up (budget);
      // what the probes read: the slice's LL samples, the reconstructed row above (from one sample to the left) and the
      // reconstructed column to the left, all final (their slices lie on earlier diagonals)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int kc = c ? 1 : 0;
        const void *plane = c == 0 ? job.comp[0] : c == 1 ? job.comp[1] : job.comp[2];
        const int stride = c == 0 ? job.stride[0] : c == 1 ? job.stride[1] : job.stride[2];
        const EncRect r = enc_rect (plane, stride, kc ? P.iwt_cw : P.iwt_lw, kc ? P.iwt_ch : P.iwt_lh, P.depth, 0, sx, sy, P.nh, P.nv);
        const int16_t *rec = job.recon + L.recon_off[c];
        const int w = llw[kc];
        for (int y = 0; y < r.bh; y++)
          for (int x = 0; x < r.bw; x++)
            buf[(L.coef[c] + y * r.bw + x) * T + tid] = (int16_t) enc_sample (r, x, y);
        for (int x = -1; x < r.bw; x++)
          buf[(L.top[c] + 1 + x) * T + tid] = r.ymin > 0 && r.xmin + x >= 0 ? gload < int16_t > (rec + (size_t) (r.ymin - 1) * w + r.xmin + x) : (int16_t) 0;
        for (int y = 0; y < r.bh; y++)
          buf[(L.left[c] + y) * T + tid] = r.xmin > 0 ? gload < int16_t > (rec + (size_t) (r.ymin + y) * w + r.xmin - 1) : (int16_t) 0;
      }
      const uint32_t *est = job.est + (size_t) s * 130;
      int i = 0, chosen = -1;
#pragma unroll 1
      for (int step = 0; chosen < 0; step++) {
        // :1116-1148: index 0 stays if it fits (<=); sizes 32 .. 1 move up while the estimate reaches the budget (>=); i + 1
        const int b = step == 0 ? 0 : step < 7 ? i + (64 >> step) : i + 1;
        const bool last = step == 7;
        const int qi = min (max (b - q0, 0), 60);
        const uint32_t factor = kEncQuant.factor[qi], qoffset = kEncQuant.offset[qi];
        uint32_t total[3];
        int lastnz[3], count[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const int kc = c ? 1 : 0;
          const int w = llw[kc], h = llh[kc];
          const int xmin = (w * sx) / P.nh, bw = (w * (sx + 1)) / P.nh - xmin;
          const int ymin = (h * sy) / P.nv, bh = (h * (sy + 1)) / P.nv - ymin;
          int16_t *rec = job.recon + L.recon_off[c];
          uint32_t bits = 0;
          int nz = -1, n = 0;
          for (int y = 0; y < bh; y++) {
            int32_t upleft = y == 0 ? buf[L.top[c] * T + tid] : buf[(L.left[c] + y - 1) * T + tid];
            int32_t left = buf[(L.left[c] + y) * T + tid];
            for (int x = 0; x < bw; x++, n++) {
              const int32_t up = y == 0 ? buf[(L.top[c] + 1 + x) * T + tid] : buf[(L.row + x) * T + tid];
              const int32_t pred = dc_pred (xmin + x, ymin + y, left, up, upleft);
              const int32_t v = buf[(L.coef[c] + n) * T + tid];
              const int32_t q = w16 (enc_quantise (v - pred, factor, qoffset));
              const int32_t rv = w16 (pred + enc_dequantise (q, factor, qoffset));
              bits += (uint32_t) sint_bits (q);
              nz = q ? n : nz;
              buf[(L.row + x) * T + tid] = (int16_t) rv;
              if (step == 0 || last)    // (index 0 is final when it fits)
                gstore < int16_t > (rec + (size_t) (ymin + y) * w + xmin + x, (int16_t) rv);
              upleft = up;
              left = rv;
            }
          }
          total[c] = bits;
          lastnz[c] = nz;
          count[c] = n;
        }
        // :990-996, :1050-1061: bits minus trailing zeros (a zero is one bit), luma over the whole array, chroma in pairs
        const uint32_t hy = gload < uint32_t > (est + 2 * b), hc = gload < uint32_t > (est + 2 * b + 1);
        const uint32_t ny = hy ? total[0] + hy : total[0] - (uint32_t) (count[0] - 1 - lastnz[0]);
        const uint32_t nc = hc ? total[1] + total[2] + hc
            : total[1] + total[2] - 2u * (uint32_t) (count[1] - 1 - max (lastnz[1], lastnz[2]));
        const uint32_t nbits = header + ny + nc;
        if (step == 0) {
          if (nbits <= budget)
            chosen = 0;
        } else if (last) {
          chosen = b;
        } else if (nbits >= budget) {
          i = b;
        }
      }
      gstore < uint8_t > (job.index + s, (uint8_t) chosen);
    }
    __syncthreads ();           // the next diagonal reads this one's reconstruction (one workgroup: one CU, one L1)
  }
}

// ---- pack -------------------------------------------------------------------------------------------------------------

struct PackState {
  uint32_t *wbase;              // the 4-byte aligned word at or before the slice's first byte
  uint32_t first_byte, end_byte;        // the slice, in bytes from wbase
  uint32_t pos;                 // bits from wbase written so far
};

// word w (counted from wbase) of the stream, `value` big-endian: whole if the slice covers it, else its bytes inside
__device__ __forceinline__ void
pack_store_word (const PackState & st, uint32_t w, uint32_t value)
{
  const uint32_t b0 = 4u * w;
  if (b0 >= st.first_byte && b0 + 4u <= st.end_byte) {
    gstore < uint32_t > (st.wbase + w, __builtin_bswap32 (value));
    return;
  }
#pragma unroll
  for (uint32_t k = 0; k < 4; k++)
    if (b0 + k >= st.first_byte && b0 + k < st.end_byte)
      gstore < uint8_t > ((uint8_t *) st.wbase + b0 + k, (uint8_t) (value >> (24u - 8u * k)));
}

// every lane's code (len 0: none) behind the bits written so far; returns the lane's first bit
__device__ __forceinline__ uint32_t
pack_emit (PackState & st, uint32_t * win, uint32_t code, int len, int lane)
{
  uint32_t incl = (uint32_t) len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t) __shfl_up ((int) incl, d);
    incl += lane >= d ? o : 0u;
  }
  const uint32_t total = (uint32_t) __shfl ((int) incl, 63);
  const uint32_t w0 = st.pos >> 5;
  const uint32_t mine = st.pos + incl - (uint32_t) len;
  if (len) {
    const uint32_t rel = mine - (w0 << 5), sh = rel & 31u;
    const uint64_t v = (((uint64_t) code) << (64 - len)) >> sh;
    atomicOr (&win[rel >> 5], (uint32_t) (v >> 32));
    if (sh + (uint32_t) len > 32u)
      atomicOr (&win[(rel >> 5) + 1], (uint32_t) v);
  }
  __syncthreads ();
  const uint32_t pos1 = st.pos + total;
  const uint32_t nfull = (pos1 >> 5) - w0;      // <= 64 whole words
  const uint32_t mine_w = (uint32_t) lane < nfull ? win[lane] : 0u;
  const uint32_t carry = win[nfull];
  if ((uint32_t) lane < nfull && 4u * (w0 + (uint32_t) lane) < st.end_byte)
    pack_store_word (st, w0 + (uint32_t) lane, mine_w);
  __syncthreads ();
  for (int k = lane; k < kWinWords; k += 64)
    win[k] = 0;
  __syncthreads ();
  if (lane == 0)
    win[0] = carry;
  __syncthreads ();
  st.pos = pos1;
  return mine;
}

__device__ __forceinline__ int32_t
wave_sum (int32_t v)
{
#pragma unroll
  for (int d = 32; d; d >>= 1)
    v += __shfl_xor (v, d);
  return v;
}

__device__ __forceinline__ int32_t
wave_max (int32_t v)
{
#pragma unroll
  for (int d = 32; d; d >>= 1)
    v = max (v, __shfl_xor (v, d));
  return v;
}

// the quantised value of sample (x, y) of the slice's rectangle r in sub-band `index` of component c
__device__ __forceinline__ int32_t
pack_value (const EncJob & job, int recon_off, const EncRect & r, int index, int llw, int x, int y,
    uint32_t factor, uint32_t qoffset)
{
  const int32_t v = enc_sample (r, x, y);
  if (index)
    return enc_quantise (v, factor, qoffset);
  const int16_t *rec = job.recon + recon_off;
  const int X = r.xmin + x, Y = r.ymin + y;
  const int32_t left = X > 0 ? gload < int16_t > (rec + (size_t) Y * llw + X - 1) : 0;
  const int32_t up = Y > 0 ? gload < int16_t > (rec + (size_t) (Y - 1) * llw + X) : 0;
  const int32_t upleft = X > 0 && Y > 0 ? gload < int16_t > (rec + (size_t) (Y - 1) * llw + X - 1) : 0;
  return w16 (enc_quantise (v - dc_pred (X, Y, left, up, upleft), factor, qoffset));
}

__global__ __launch_bounds__ (64)
void ldenc_pack_kernel (const EncJob * __restrict__ jobs, const SliceParams P, const int recon_u, const int recon_v)
{
  __shared__ uint32_t win[kWinWords];
  const EncJob & job = jobs[blockIdx.y];      // (members are read where they are used)
  const int lane = (int) threadIdx.x;
  const int s = (int) blockIdx.x;
  const int sy = s / P.nh, sx = s - sy * P.nh;
  const int nsub = 1 + 3 * P.depth;
  uint32_t offset, slice_bytes;
  enc_slice_bytes (P, s, &offset, &slice_bytes);
  const int base_index = gload < uint8_t > (job.index + s);
  for (int k = lane; k < kWinWords; k += 64)
    win[k] = 0;
  __syncthreads ();

  PackState st;
  const uintptr_t addr = (uintptr_t) job.out + offset;
  st.wbase = (uint32_t *) (addr & ~(uintptr_t) 3);
  st.first_byte = (uint32_t) (addr & 3);
  st.end_byte = st.first_byte + slice_bytes;
  st.pos = 8u * st.first_byte;
  const uint32_t start = st.pos, end = 8u * st.end_byte;
  const int llw_y = P.iwt_lw >> P.depth, llw_c = P.iwt_cw >> P.depth;

  // pass 1 over luma: slice_y_length = bits up to the last non-zero value of the whole array (:802)
  int32_t bits = 0, lastnz = -1, ny = 0;
#pragma unroll 1
  for (int i = 0; i < nsub; i++) {
    const int qi = min (max (base_index - P.quant_matrix[i], 0), 60);
    const uint32_t factor = kEncQuant.factor[qi], qoffset = kEncQuant.offset[qi];
    const EncRect r = enc_rect (job.comp[0], job.stride[0], P.iwt_lw, P.iwt_lh, P.depth, i, sx, sy, P.nh, P.nv);
    const int n = r.bw * r.bh;
    for (int e = lane; e < n; e += 64) {
      const int y = e / r.bw, x = e - y * r.bw;
      const int32_t q = pack_value (job, 0, r, i, llw_y, x, y, factor, qoffset);
      bits += sint_bits (q);
      lastnz = q ? ny + e : lastnz;
    }
    ny += n;
  }
  lastnz = wave_max (lastnz);
  const uint32_t y_length = (uint32_t) (wave_sum (bits) - (ny - 1 - lastnz));

  // the header: 7 bits of base index, ilog2up (8 slice_bytes) bits of slice_y_length (:799-803)
  {
    const int length_bits = enc_ilog2up (8u * slice_bytes);
    const uint32_t field = length_bits >= 32 ? y_length : y_length & ((1u << length_bits) - 1u);
    pack_emit (st, win, lane == 0 ? (uint32_t) base_index : field, lane == 0 ? 7 : lane == 1 ? length_bits : 0, lane);
  }
  // luma up to the last non-zero value (:805-807)
  int done = 0;
#pragma unroll 1
  for (int i = 0; i < nsub && done <= lastnz; i++) {
    const int qi = min (max (base_index - P.quant_matrix[i], 0), 60);
    const uint32_t factor = kEncQuant.factor[qi], qoffset = kEncQuant.offset[qi];
    const EncRect r = enc_rect (job.comp[0], job.stride[0], P.iwt_lw, P.iwt_lh, P.depth, i, sx, sy, P.nh, P.nv);
    const int n = r.bw * r.bh;
#pragma unroll 1
    for (int c0 = 0; c0 < n && done + c0 <= lastnz; c0 += 64) {
      const int e = c0 + lane;
      int len = 0;
      uint32_t code = 0;
      if (e < n && done + e <= lastnz) {
        const int y = e / r.bw, x = e - y * r.bw;
        code = sint_code (pack_value (job, 0, r, i, llw_y, x, y, factor, qoffset), &len);
      }
      pack_emit (st, win, code, len, lane);
    }
    done += n;
  }
  // chroma, U and V value by value (:809-815).  Every pair is written: the zero pairs behind the last non-zero one are
  // 1-bits, which is what the padding puts there; `used` is where the reference's slice ends
  uint32_t used = st.pos;
#pragma unroll 1
  for (int i = 0; i < nsub; i++) {
    const int qi = min (max (base_index - P.quant_matrix[i], 0), 60);
    const uint32_t factor = kEncQuant.factor[qi], qoffset = kEncQuant.offset[qi];
    const EncRect ru = enc_rect (job.comp[1], job.stride[1], P.iwt_cw, P.iwt_ch, P.depth, i, sx, sy, P.nh, P.nv);
    const EncRect rv = enc_rect (job.comp[2], job.stride[2], P.iwt_cw, P.iwt_ch, P.depth, i, sx, sy, P.nh, P.nv);
    const int n = 2 * ru.bw * ru.bh;
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int e = c0 + lane;
      int len = 0;
      uint32_t code = 0;
      int32_t q = 0;
      if (e < n) {
        const int p = e >> 1, y = p / ru.bw, x = p - y * ru.bw;
        q = (e & 1) ? pack_value (job, recon_v, rv, i, llw_c, x, y, factor, qoffset)
            : pack_value (job, recon_u, ru, i, llw_c, x, y, factor, qoffset);
        code = sint_code (q, &len);
      }
      const uint32_t at = pack_emit (st, win, code, len, lane);
      // a non-zero value closes its pair: the U of a pair with a zero V still carries that V's one bit
      const uint32_t pair_end = at + (uint32_t) len + ((e & 1) == 0 && e < n ? 1u : 0u);
      used = max (used, (uint32_t) wave_max (q ? (int32_t) pair_end : 0));
    }
  }
  if (used > end) {
    // the reference asserts (:826-830); here the slice is cut at its last bit and counted
    if (lane == 0)
      __hip_atomic_fetch_add ((SCHRO_GLOBAL uint32_t *) job.overrun, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    // 1-bits up to the slice's end (:832-835)
#pragma unroll 1
    while (st.pos < end) {
      const uint32_t rem = end - st.pos;
      const int len = (int) min (32u, rem > 32u * (uint32_t) lane ? rem - 32u * (uint32_t) lane : 0u);
      pack_emit (st, win, len == 32 ? 0xffffffffu : (1u << len) - 1u, len, lane);
    }
  }
  // the bits of the last, partial word
  if (lane == 0 && 4u * (st.pos >> 5) < st.end_byte && st.pos > start)
    pack_store_word (st, st.pos >> 5, win[0]);
}

}                               // namespace

int
launch_lowdelay_encode (hipStream_t stream, const EncJob * d_jobs, int njobs, const SliceParams & P, const EncChooseLayout & L,
    int stages)
{
  const int nslices = P.nh * P.nv;
  if (stages & 1)
    SCHRO_LAUNCH (ldenc_estimate_kernel, dim3 (nslices, njobs), dim3 (64), 0, stream, d_jobs, P);
  if (stages & 2)
    SCHRO_LAUNCH (ldenc_choose_kernel, dim3 (njobs), dim3 (L.threads), (size_t) L.lds_bytes, stream, d_jobs, P, L);
  if (stages & 4)
    SCHRO_LAUNCH (ldenc_pack_kernel, dim3 (nslices, njobs), dim3 (64), 0, stream, d_jobs, P, L.recon_off[1], L.recon_off[2]);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "lowdelay encode launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
