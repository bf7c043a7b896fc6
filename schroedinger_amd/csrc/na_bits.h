// na_bits.h -- the bit writer the VLC (noarith) encoders share on the device (noarith_enc.hip, motion_enc.hip): the output
// window of a picture with the bytes that belong to it as masks, bits OR-ed into the cleared output, and the parse codes
// of schropack.c:148-178.
#pragma once

#include "schro_hip_internal.h"

namespace schro {
namespace {

struct NaOut {
  uint32_t *wbase;              // the 4-byte aligned word at or before the picture's first byte
  uint32_t first_byte, end_byte;        // the output, in bytes from wbase
};

// the bytes of word w (counted from wbase) that belong to the output, as a mask over the big-endian value
__device__ __forceinline__ uint32_t
na_mask (const NaOut & st, uint32_t w)
{
  const uint32_t b0 = 4u * w;
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++)
    if (b0 + k >= st.first_byte && b0 + k < st.end_byte)
      m |= 0xff000000u >> (8u * k);
  return m;
}

// OR `value` (big-endian: bit 31 is the word's first bit) into word w; the output was cleared
__device__ __forceinline__ void
na_or_word (const NaOut & st, uint32_t w, uint32_t value)
{
  value &= na_mask (st, w);
  if (value)
    __hip_atomic_fetch_or ((SCHRO_GLOBAL uint32_t *) (st.wbase + w), __builtin_bswap32 (value), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT);
}

// `len` bits (0 .. 64), right-aligned in `code`, at bit `pos` from wbase
__device__ __forceinline__ void
na_or_bits (const NaOut & st, uint32_t pos, uint64_t code, int len)
{
  if (len <= 0)
    return;
  const uint64_t v = code << (64 - len);
  const uint32_t sh = pos & 31u, w = pos >> 5;
  const uint32_t hi = (uint32_t) (v >> 32), lo = (uint32_t) v;
  na_or_word (st, w, hi >> sh);
  na_or_word (st, w + 1, sh ? (hi << (32u - sh)) | (lo >> sh) : lo);
  if (sh)
    na_or_word (st, w + 2, lo << (32u - sh));
}

// bit i of x to bit 2 i
__device__ __forceinline__ uint64_t
na_spread (uint32_t x32)
{
  uint64_t x = x32;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// schro_pack_encode_uint (schropack.c:148-161) of value < 2^32 - 1: right-aligned, 1 .. 63 bits
__device__ __forceinline__ uint64_t
na_uint_code (uint32_t value, int *len)
{
  const uint64_t v = (uint64_t) value + 1u;
  const int l = 64 - __clzll ((long long) v);
  *len = 2 * l - 1;
  return (na_spread ((uint32_t) (v & (((uint64_t) 1 << (l - 1)) - 1u))) << 1) | 1u;
}

__device__ __forceinline__ uint32_t
na_mag (int32_t q)
{
  return q < 0 ? 0u - (uint32_t) q : (uint32_t) q;
}

// schro_pack_encode_sint (:163-178): 1 .. 64 bits (INT_MIN, undefined in the reference, codes magnitude 2^31)
__device__ __forceinline__ int
na_sint_bits (int32_t q)
{
  const uint32_t mag = na_mag (q);
  const int l = 64 - __clzll ((long long) ((uint64_t) mag + 1u));
  return 2 * l - 1 + (mag ? 1 : 0);
}

__device__ __forceinline__ uint64_t
na_sint_code (int32_t q, int *len)
{
  int l;
  const uint64_t u = na_uint_code (na_mag (q), &l);
  if (q == 0) {
    *len = l;
    return u;
  }
  *len = l + 1;
  return (u << 1) | (q < 0 ? 1u : 0u);
}

}                               // namespace
}                               // namespace schro
