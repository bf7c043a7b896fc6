// arith_bin.h -- the binary arithmetic decoder of the core syntax (schroarith.h:147-196, schroarith.c:211-239), shared by
// arith_dec.hip and motion_arith_dec.hip: the coder's state over a payload of any alignment (0xff behind its end) and one bin
// against a probability and the 256-entry update table its caller holds (each file states the table: the tests pin both
// against tests/golden/arith_lut.json).  Moved out of arith_dec.hip; the source of the bytes became a template parameter.
#pragma once

#include "schro_hip_internal.h"
#include "na_chunks.h"

namespace schro {
namespace {

// ---- the coder ---------------------------------------------------------------------------------------------------------

struct AdCoder {
  uint32_t range, code;
  uint32_t offset;              // of the last byte taken
  uint32_t cntr;
};

// byte `off` of the payload; 0xff behind its end (schroarith.h:162-173)
__device__ __forceinline__ uint32_t
ad_byte (const NdBits & B, uint32_t off)
{
  const uint32_t at = B.first + off;
  if (at >= B.end)
    return 0xffu;
  return (nd_word (B, at >> 2) >> (24u - 8u * (at & 3u))) & 0xffu;
}

// schro_arith_decode_init.  Bytes: whatever ad_byte reads a payload's byte from -- NdBits (global memory), or a window of it
// a wave keeps in LDS (motion_arith_dec.hip)
template < typename Bytes > __device__ __forceinline__ void
ad_init (AdCoder & a, const Bytes & B)
{
  a.range = 0xffff0000u;
  a.code = (ad_byte (B, 0) << 24) | (ad_byte (B, 1) << 16) | (ad_byte (B, 2) << 8) | ad_byte (B, 3);
  a.offset = 3;
  a.cntr = 16;
}

// _schro_arith_decode_bit with the probability in *p.  The renormalisation loop shifts one bit at a time while
// range <= 0x40000000; here the number of shifts comes from the range's leading zeros and they are taken in runs that end
// where two bytes enter.  range is never 0: its low 16 bits are, p stays within 0xfe .. 0xff01 (lut[0] is 0), and
// (range >> 16) >= 0x4001 behind the renormalisation.  A bin shifts 15 times at the most (range >= 0x10000) and so takes at
// most the two bytes behind `offset`.
template < typename Bytes, typename P > __device__ __forceinline__ uint32_t
ad_bin (AdCoder & a, const Bytes & B, P * p, const uint16_t * lut)
{
  uint32_t range = a.range, code = a.code;
  if (range <= 0x40000000u) {
    const uint32_t k = 31u - (uint32_t) __clz ((int) range);
    uint32_t s = 30u - k + ((range & (range - 1u)) == 0u ? 1u : 0u);
#pragma unroll 1
    while (s) {
      const uint32_t n = min (s, a.cntr);
      range <<= n;
      code <<= n;
      s -= n;
      a.cntr -= n;
      if (a.cntr == 0) {
        code |= (ad_byte (B, a.offset + 1) << 8) | ad_byte (B, a.offset + 2);
        a.offset += 2;
        a.cntr = 16;
      }
    }
  }
  const uint32_t prob = *p;
  const uint32_t rxp = ((range >> 16) * prob) & 0xffff0000u;
  const uint32_t bit = code >= rxp ? 1u : 0u;
  *p = (P) (bit ? prob - lut[prob >> 8] : prob + lut[255u - (prob >> 8)]);
  a.code = bit ? code - rxp : code;
  a.range = bit ? range - rxp : rxp;
  return bit;
}

}                               // namespace
}                               // namespace schro
