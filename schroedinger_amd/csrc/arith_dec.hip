// arith_dec.hip -- arithmetic-coded core-syntax transform data, read on the device: the twin of
// schro_decoder_decode_transform_data (schrodecoder.c:2990-3015) for !is_noarith over schro_decoder_decode_subband
// (:3525-3638), schro_decoder_decode_codeblock (:3452-3522), the generic line decoder (:3018-3217) and the binary
// arithmetic decoder (schroarith.h:147-210, schroarith.c:211-239, 283-288, 642-668).  schro_hip.h states the rules.
//
// Every bin depends on the one before it, so a sub-band is one serial chain, and sub-band i >= 4 reads sub-band i - 3 of
// its component (the parent's zero test).  What is independent is the TOWER: the LL band of a component, and per
// orientation the bands from the coarsest level to the finest -- four per component, twelve per picture.
//
//   ad_header_kernel  thread 0 of a wave per picture walks the sub-band headers (the VLC codes of na_chunks.h, as
//                     nd_header_kernel does), cuts payloads at the input's end and runs the compat test: a sint peeked on a
//                     fresh coder of sub-band 0's payload.
//   ad_clear_kernel   zeroes the planes (widths, not strides) of every picture without the error: zero sub-bands and zero
//                     codeblocks are then zero to their children and neighbours, and a value of 0 needs no store.
//   ad_decode_kernel  a wave per tower with lane 0 deciding, as a state machine that decodes ONE BIN PER TRIP of its loop;
//                     what differs from trip to trip -- which context, what the bit means -- is bookkeeping around the
//                     bin.  The 22 probabilities of a chain sit in LDS as [context][lane], the 256-entry table beside
//                     them.  Neighbours and parents are read back from the plane -- the STORED values, truncated to the
//                     sample type --; within a row the left and upper-left values are carried in registers as stored.
//                     The same kernel runs a LANE per tower (64 unlike chains of a wave sharing the bin's instructions,
//                     towers of like length side by side) in the experiments build: measured to take 24 to 37 % longer on the
//                     reference's stream (profiles/arith_decode.txt).  A call holds at most kMaxJobs pictures,
//                     3072 towers: fewer waves than are resident on the device at this kernel's occupancy.
//
// Nothing is read outside the aligned dwords that hold the input's bytes, and nothing of a picture whose header walk set
// the error is written.  No trip count has a cap of its own: DESIGN 4.24 gives the bound that follows from the input.
//
// Dequantisation is C int for both sample sizes (schrodecoder.c:3072-3079), not dequant_one.h's 16-bit Orc form.  Where C
// leaves offset + factor * v + 2 undefined (overflow) this computes the 32-bit two's-complement wrap, an arithmetic shift
// and a wrapping negation: what the x86-64 build of the reference does, and not pinned against it.

#include "schro_hip_internal.h"
#include "dequant_one.h"
#include "na_chunks.h"
#include "arith_bin.h"

namespace schro {
namespace {

// Dirac specification, the arithmetic decoder's probability update table (256 entries); pinned against the reference's
// numbers by tests/test_arith_dec_ref.py (tests/golden/arith_lut.json)
static __device__ __constant__ uint16_t kAdLut[256] = {
  0, 2, 5, 8, 11, 15, 20, 24, 29, 35, 41, 47, 53, 60, 67, 74,
  82, 89, 97, 106, 114, 123, 132, 141, 150, 160, 170, 180, 190, 201, 211, 222,
  233, 244, 256, 267, 279, 291, 303, 315, 327, 340, 353, 366, 379, 392, 405, 419,
  433, 447, 461, 475, 489, 504, 518, 533, 548, 563, 578, 593, 609, 624, 640, 656,
  672, 688, 705, 721, 738, 754, 771, 788, 805, 822, 840, 857, 875, 892, 910, 928,
  946, 964, 983, 1001, 1020, 1038, 1057, 1076, 1095, 1114, 1133, 1153, 1172, 1192, 1211, 1231,
  1251, 1271, 1291, 1311, 1332, 1352, 1373, 1393, 1414, 1435, 1456, 1477, 1498, 1520, 1541, 1562,
  1584, 1606, 1628, 1649, 1671, 1694, 1716, 1738, 1760, 1783, 1806, 1828, 1851, 1874, 1897, 1920,
  1935, 1942, 1949, 1955, 1961, 1968, 1974, 1980, 1985, 1991, 1996, 2001, 2006, 2011, 2016, 2021,
  2025, 2029, 2033, 2037, 2040, 2044, 2047, 2050, 2053, 2056, 2058, 2061, 2063, 2065, 2066, 2068,
  2069, 2070, 2071, 2072, 2072, 2072, 2072, 2072, 2072, 2071, 2070, 2069, 2068, 2066, 2065, 2063,
  2060, 2058, 2055, 2052, 2049, 2045, 2042, 2038, 2033, 2029, 2024, 2019, 2013, 2008, 2002, 1996,
  1989, 1982, 1975, 1968, 1960, 1952, 1943, 1934, 1925, 1916, 1906, 1896, 1885, 1874, 1863, 1851,
  1839, 1827, 1814, 1800, 1786, 1772, 1757, 1742, 1727, 1710, 1694, 1676, 1659, 1640, 1622, 1602,
  1582, 1561, 1540, 1518, 1495, 1471, 1447, 1422, 1396, 1369, 1341, 1312, 1282, 1251, 1219, 1186,
  1151, 1114, 1077, 1037, 995, 952, 906, 857, 805, 750, 690, 625, 553, 471, 376, 255,
};

// the contexts of transform data, in the order of the reference's enum (SCHRO_CTX_ZERO_CODEBLOCK .. SCHRO_CTX_COEFF_DATA)
enum {
  kCtxZeroCodeblock = 0, kCtxQCont = 1, kCtxQValue = 2, kCtxQSign = 3,
  kCtxZpznF1 = 4, kCtxZpnnF1 = 5, kCtxZpF2 = 6, kCtxZpF6 = 10,
  kCtxNpznF1 = 11, kCtxNpnnF1 = 12, kCtxNpF2 = 13, kCtxNpF6 = 17,
  kCtxSignPos = 18, kCtxSignNeg = 19, kCtxSignZero = 20, kCtxCoeffData = 21,
};
static_assert (kCtxCoeffData + 1 == kAdContexts, "the contexts of a chain");

// next_list (schroarith.c) for the continuation contexts above: F1 (either) -> F2 -> ... -> F6 -> F6; the quantiser's stays
__device__ __forceinline__ uint32_t
ad_follow (uint32_t c)
{
  const uint32_t step = (c == kCtxZpznF1 || c == kCtxNpznF1) ? 2u : (c == kCtxQCont || c == kCtxZpF6 || c == kCtxNpF6) ? 0u : 1u;
  return c + step;
}

// ---- header ------------------------------------------------------------------------------------------------------------

// _schro_arith_decode_sint (QUANTISER_CONT, _VALUE, _SIGN) on a fresh coder of the payload: the compat test's peek
__device__ int32_t
ad_peek_sint (const NdBits & B)
{
  AdCoder a;
  ad_init (a, B);
  uint32_t pc = 0x8000u, pv = 0x8000u, ps = 0x8000u, bits = 1;
  int count = 0;
#pragma unroll 1
  while (!ad_bin (a, B, &pc, kAdLut)) {
    bits = (bits << 1) | ad_bin (a, B, &pv, kAdLut);
    if (++count == 30)
      break;
  }
  int32_t v = (int32_t) (bits - 1u);
  if (v && ad_bin (a, B, &ps, kAdLut))
    v = -v;
  return v;
}

__global__ __launch_bounds__ (64)
void ad_header_kernel (const NdSubband * __restrict__ sbs, const AdPicture * __restrict__ pics, AdBand * __restrict__ bands)
{
  if (threadIdx.x != 0)
    return;
  const AdPicture & pic = pics[blockIdx.x];
  SchroHipArithDecodeResult *res = pic.result;
  uint32_t L = pic.data_bytes;
  if (pic.bytes_on_device)
    L = min (L, gload < uint32_t > (pic.bytes_on_device));
  const NdBits O = nd_bits (pic.data, 0, L);
  uint64_t pos = 0;
  uint32_t longs = 0, truncated = 0, error = 0, compat = pic.compat ? 1u : 0u;
#pragma unroll 1
  for (int s = 0; s < pic.nsb; s++) {
    const NdSubband & sb = sbs[pic.sb_first + s];
    AdBand band;
    band.first_byte = band.bytes = band.length = band.quant_index = band.flags = band.pad[0] = band.pad[1] = band.pad[2] = 0;
    if (!error) {
      pos = (pos + 7u) & ~7ull;
      const uint32_t length = nd_code (O, pos, longs, false);
      if (length == 0) {
        pos = (pos + 7u) & ~7ull;
      } else {
        const uint32_t qi = nd_code (O, pos, longs, false);
        if (qi > 60u) {
          error = 1;
          gstore < uint32_t > (&res->error, 1u);
          gstore < uint32_t > (&res->first_error, (uint32_t) (sb.comp * SCHRO_HIP_NOARITH_MAX_SUBBANDS + sb.index));
        } else {
          pos = (pos + 7u) & ~7ull;
          const uint64_t fb = pos >> 3;
          const uint32_t avail = fb < L ? min (length, L - (uint32_t) fb) : 0u;
          truncated += avail < length;
          pos += 8ull * length;
          const bool one = sb.hc == 1 && sb.vc == 1;
          bool qo = pic.mode == 1 && !(compat && one);
          // schro_decoder_test_quant_offset_compat: a sub-band of one codeblock has no zero flag in front of the offset
          if (qo && one && sb.index == 0) {
            const int64_t q = (int64_t) qi + ad_peek_sint (nd_bits (pic.data, avail ? (uint32_t) fb : 0u, avail));
            if (q < 0 || q > 60) {
              compat = 1;
              qo = false;
            }
          }
          band.first_byte = avail ? (uint32_t) fb : 0u;
          band.bytes = avail;
          band.length = length;
          band.quant_index = qi;
          band.flags = 1u | (one ? 0u : 2u) | (qo ? 4u : 0u);
          gstore < uint32_t > (&res->subband_length[sb.comp][sb.index], length);
          gstore < uint8_t > (&res->subband_quant_index[sb.comp][sb.index], (uint8_t) qi);
        }
      }
    }
    uint32_t *out = (uint32_t *) (bands + pic.sb_first + s);
    const uint32_t *in = (const uint32_t *) &band;
#pragma unroll
    for (int k = 0; k < kAdBandWords; k++)
      gstore < uint32_t > (out + k, in[k]);
  }
  if (!error)
    pos = (pos + 7u) & ~7ull;
  const uint64_t bytes_read = (pos + 7u) >> 3;
  gstore < uint32_t > (&res->bytes_read, bytes_read > 0xffffffffull ? 0xffffffffu : (uint32_t) bytes_read);
  gstore < uint32_t > (&res->compat_quant_offset, error ? (pic.compat ? 1u : 0u) : compat);
  gstore < uint32_t > (&res->truncated, truncated);
  gstore < uint32_t > (&res->long_codes, longs);
}

// ---- clear -------------------------------------------------------------------------------------------------------------

template < typename T >
__global__ __launch_bounds__ (256)
void ad_clear_kernel (const AdPicture * __restrict__ pics)
{
  const AdPicture & pic = pics[blockIdx.y / 3];
  const int k = (int) (blockIdx.y % 3);
  if (gload < uint32_t > (&pic.result->error))
    return;
  const int w = pic.width[k], h = pic.height[k];
#pragma unroll 1
  for (int y = (int) blockIdx.x; y < h; y += (int) gridDim.x) {
    const size_t at = (size_t) y * (size_t) pic.stride[k];
    for (int x = (int) threadIdx.x; x < w; x += (int) blockDim.x) {
      gstore < T > ((T *) ((char *) pic.coeffs[k] + at) + x, (T) 0);
      if (pic.quant[k])
        gstore < T > ((T *) ((char *) pic.quant[k] + at) + x, (T) 0);
    }
  }
}

// ---- decode ------------------------------------------------------------------------------------------------------------

// what a lane does next.  The first four take no bin.
enum {
  kPhBand,                      // the tower's next sub-band
  kPhCodeblock,                 // codeblock (cx, cy) of the band, or the band's end
  kPhOffset,                    // behind the zero flag
  kPhValues,                    // behind the quant offset
  kPhDone,
  kPhZero, kPhQCont, kPhQValue, kPhQSign, kPhCont, kPhValue, kPhSign,
};

// bins += n, saturating
__device__ __forceinline__ void
ad_add_sat (uint32_t * p, uint64_t n)
{
  uint32_t old = gload < uint32_t > (p);
#pragma unroll 1
  for (;;) {
    const uint64_t sum = (uint64_t) old + n;
    const uint32_t want = sum > 0xffffffffull ? 0xffffffffu : (uint32_t) sum;
    const uint32_t seen = atomicCAS (p, old, want);
    if (seen == old)
      break;
    old = seen;
  }
}

template < typename T >
__global__ __launch_bounds__ (64)
void ad_decode_kernel (const NdSubband * __restrict__ sbs, const AdPicture * __restrict__ pics, const AdTower * __restrict__ towers,
    int ntowers, const AdBand * __restrict__ bands, int per_lane)
{
  __shared__ uint16_t prob[kAdContexts][64];
  __shared__ uint16_t lut[256];
  const int lane = (int) threadIdx.x;
  for (int k = lane; k < 256; k += 64)
    lut[k] = kAdLut[k];
  __syncthreads ();
  const int t = per_lane ? (int) blockIdx.x * 64 + lane : lane == 0 ? (int) blockIdx.x : ntowers;
  if (t >= ntowers)
    return;
  const AdTower tw = towers[t];
  const AdPicture & pic = pics[tw.pic];
  SchroHipArithDecodeResult *res = pic.result;
  if (gload < uint32_t > (&res->error))
    return;
  const uint32_t *offsets = pic.is_intra ? kDevQuant.off12 : kDevQuant.off38;

  // the band
  int band = 0, bw = 0, bh = 0, hc = 1, vc = 1, stride = 0, pstride = 0, orient = 0;
  char *coeffs = nullptr, *quant = nullptr;
  const char *parent = nullptr;
  uint32_t flags = 0, length = 0;
  NdBits B = nd_bits (pic.data, 0, 0);
  AdCoder a = { 0xffff0000u, 0, 3, 16 };
  // the codeblock
  int cx = 0, cy = 0, xmin = 0, xmax = 0, ymin = 0, ymax = 0;
  int64_t qi = 0;
  uint32_t factor = 0, offset = 0;
  // the coefficient
  int i = 0, j = 0;
  int32_t left = 0, up = 0, upleft = 0, v = 0;
  uint32_t cont = 0, sign = 0, bits = 1, count = 0;
  // the tower's counts
  uint64_t bins = 0;
  uint32_t longs = 0, clamped = 0, not_consumed = 0, overran = 0;
  int phase = kPhBand;

#pragma unroll 1
  for (;;) {
    if (phase == kPhBand) {
      if (band == tw.nbands) {
        phase = kPhDone;
      } else {
        const int si = tw.sb_first + 3 * band;
        const NdSubband & sb = sbs[si];
        const AdBand & bd = bands[si];
        flags = gload < uint32_t > (&bd.flags);
        if (!(flags & 1u)) {
          band++;               // a zero sub-band: cleared
          continue;
        }
        bw = sb.bw;
        bh = sb.bh;
        hc = sb.hc;
        vc = sb.vc;
        stride = sb.stride;
        coeffs = (char *) sb.coeffs;
        quant = (char *) sb.quant;
        orient = sb.index == 0 ? 0 : (sb.index - 1) % 3 + 1;
        parent = sb.index >= 4 ? (const char *) sbs[si - 3].coeffs : nullptr;
        pstride = sb.index >= 4 ? sbs[si - 3].stride : 0;
        length = gload < uint32_t > (&bd.length);
        qi = gload < uint32_t > (&bd.quant_index);
        B = nd_bits (pic.data, gload < uint32_t > (&bd.first_byte), gload < uint32_t > (&bd.bytes));
        ad_init (a, B);
#pragma unroll
        for (int c = 0; c < kAdContexts; c++)
          prob[c][lane] = 0x8000u;
        cx = cy = 0;
        phase = kPhCodeblock;
      }
    }
    if (phase == kPhCodeblock) {
      if (cy == vc) {
        // schro_arith_decode_flush and what the reference warns about (:3590-3604)
        const uint64_t end = (uint64_t) a.offset + (a.cntr < 8u ? 1u : 0u);
        not_consumed += end + 1u < (uint64_t) length;
        overran += end > (uint64_t) length + 4u;
        band++;
        phase = kPhBand;
        continue;
      }
      xmin = (int) (((int64_t) cx * bw) / hc);
      xmax = (int) (((int64_t) (cx + 1) * bw) / hc);
      ymin = (int) (((int64_t) cy * bh) / vc);
      ymax = (int) (((int64_t) (cy + 1) * bh) / vc);
      phase = (flags & 2u) ? kPhZero : kPhOffset;
    }
    if (phase == kPhOffset) {
      bits = 1;
      count = 0;
      phase = (flags & 4u) ? kPhQCont : kPhValues;
    }
    if (phase == kPhValues) {
      factor = kDevQuant.factor[qi];
      offset = offsets[qi];
      if (xmax == xmin || ymax == ymin) {
        if (++cx == hc) {
          cx = 0;
          cy++;
        }
        phase = kPhCodeblock;
        continue;
      }
      i = xmin;
      j = ymin;
      phase = kPhCont;
      cont = 0;                 // (set below)
    }
    if (phase == kPhDone)
      break;

    if (phase == kPhCont && cont == 0) {
      // a coefficient starts: its neighbours as stored, its parent
      if (i == xmin) {
        left = i > 0 ? (int32_t) gload < T > ((const T *) (coeffs + (size_t) j * stride) + i - 1) : 0;
        upleft = i > 0 && j > 0 ? (int32_t) gload < T > ((const T *) (coeffs + (size_t) (j - 1) * stride) + i - 1) : 0;
      }
      up = j > 0 ? (int32_t) gload < T > ((const T *) (coeffs + (size_t) (j - 1) * stride) + i) : 0;
      const int32_t par = parent ? (int32_t) gload < T > ((const T *) (parent + (size_t) (j >> 1) * pstride) + (i >> 1)) : 0;
      const bool nhood = (left | up | upleft) != 0;
      cont = par ? (nhood ? kCtxNpnnF1 : kCtxNpznF1) : (nhood ? kCtxZpnnF1 : kCtxZpznF1);
      const int32_t pv = orient == 2 ? left : orient == 1 ? up : 0;
      sign = pv < 0 ? kCtxSignNeg : pv > 0 ? kCtxSignPos : kCtxSignZero;
      bits = 1;
      count = 0;
    }

    // the bin
    const uint32_t ctx = phase == kPhZero ? kCtxZeroCodeblock : phase == kPhQCont ? kCtxQCont : phase == kPhQValue ? kCtxQValue
        : phase == kPhQSign ? kCtxQSign : phase == kPhCont ? cont : phase == kPhValue ? kCtxCoeffData : sign;
    const uint32_t bit = ad_bin (a, B, &prob[ctx][lane], lut);
    bins++;

    // what it meant
    bool stored = false;
    int32_t value = 0;
    switch (phase) {
      case kPhZero:
        if (bit) {
          if (++cx == hc) {
            cx = 0;
            cy++;
          }
          phase = kPhCodeblock;
        } else {
          phase = kPhOffset;
        }
        break;
      case kPhQCont:
        if (!bit) {
          phase = kPhQValue;
        } else {
          v = (int32_t) (bits - 1u);
          phase = v ? kPhQSign : kPhValues;     // (an offset of 0 leaves the index as it is)
        }
        break;
      case kPhQValue:
        bits = (bits << 1) | bit;
        phase = kPhQCont;
        if (++count == 30) {
          v = (int32_t) (bits - 1u);
          phase = kPhQSign;
        }
        break;
      case kPhQSign:
        {
          const int64_t q = qi + (bit ? -(int64_t) v : (int64_t) v);
          qi = q < 0 ? 0 : q > 60 ? 60 : q;
          clamped += q != qi;
          phase = kPhValues;
        }
        break;
      case kPhCont:
        if (!bit) {
          phase = kPhValue;
        } else {
          longs += count >= 31u;
          v = (int32_t) (bits - 1u);
          if (v)
            phase = kPhSign;
          else
            stored = true;      // 0: the plane holds it
        }
        break;
      case kPhValue:
        bits = (bits << 1) | bit;
        count = min (count + 1u, 31u);
        cont = ad_follow (cont);
        phase = kPhCont;
        break;
      default:                 // kPhSign
        {
          const uint32_t d = (uint32_t) ((int32_t) (offset + factor * (uint32_t) v + 2u) >> 2);
          const T out = (T) (int32_t) (bit ? 0u - d : d);
          const size_t at = (size_t) j * stride + (size_t) i * sizeof (T);
          gstore < T > ((T *) (coeffs + at), out);
          if (quant)
            gstore < T > ((T *) (quant + at), (T) (int32_t) (bit ? 0u - (uint32_t) v : (uint32_t) v));
          value = (int32_t) out;
          stored = true;
        }
        break;
    }
    if (stored) {
      // on to the next coefficient
      upleft = up;
      left = value;
      cont = 0;
      phase = kPhCont;
      if (++i == xmax) {
        i = xmin;
        if (++j == ymax) {
          if (++cx == hc) {
            cx = 0;
            cy++;
          }
          phase = kPhCodeblock;
        }
      }
    }
  }

  if (not_consumed)
    atomicAdd (&res->not_consumed, not_consumed);
  if (overran)
    atomicAdd (&res->overran, overran);
  if (longs)
    atomicAdd (&res->long_codes, longs);
  if (clamped)
    atomicAdd (&res->clamped_quant, clamped);
  if (bins)
    ad_add_sat (&res->bins, bins);
}

}                               // namespace

int
launch_arith_decode (hipStream_t stream, const NdSubband * d_sbs, const AdPicture * d_pics, int npics, const AdTower * d_towers,
    int ntowers, AdBand * bands, int bpp, int stages, int per_lane)
{
  const int waves = per_lane ? (ntowers + 63) / 64 : ntowers;
  if (stages & 1)
    SCHRO_LAUNCH (ad_header_kernel, dim3 (npics), dim3 (64), 0, stream, d_sbs, d_pics, bands);
  if (bpp == 2) {
    if (stages & 2)
      SCHRO_LAUNCH ((ad_clear_kernel < int16_t >), dim3 (kAdClearGridX, 3 * npics), dim3 (256), 0, stream, d_pics);
    if (stages & 4)
      SCHRO_LAUNCH ((ad_decode_kernel < int16_t >), dim3 (waves), dim3 (64), 0, stream, d_sbs, d_pics, d_towers, ntowers, bands, per_lane);
  } else {
    if (stages & 2)
      SCHRO_LAUNCH ((ad_clear_kernel < int32_t >), dim3 (kAdClearGridX, 3 * npics), dim3 (256), 0, stream, d_pics);
    if (stages & 4)
      SCHRO_LAUNCH ((ad_decode_kernel < int32_t >), dim3 (waves), dim3 (64), 0, stream, d_sbs, d_pics, d_towers, ntowers, bands, per_lane);
  }
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "arith decode launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
