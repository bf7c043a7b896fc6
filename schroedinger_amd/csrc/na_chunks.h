// na_chunks.h -- the VLC parse codes read in 64-bit chunks, shared by noarith_dec.hip and motion_dec.hip: the bits of a
// payload of any alignment (guard bit 1 behind its end), one code at a bit position (schro_unpack_decode_uint / _sint as
// schro_hip.h defines them past count 30), the four-state machine over one chunk and the composition of its summaries.
// Moved unchanged out of noarith_dec.hip, whose header comment says what the states are.
#pragma once

#include "schro_hip_internal.h"

namespace schro {
namespace {

enum { kA = 0, kD = 1, kF = 2, kS = 3 };
constexpr uint64_t kFollow = 0xaaaaaaaaaaaaaaaaull;     // the follow bits of (follow, data) pairs from a window's first bit

// ---- the bits --------------------------------------------------------------------------------------------------------

struct NdBits {
  const uint32_t *wbase;        // the 4-byte aligned word at or before the first byte
  uint32_t first, end;          // the bytes, counted from wbase: [first, end)
};

__device__ __forceinline__ NdBits
nd_bits (const uint8_t * data, uint32_t first_byte, uint32_t bytes)
{
  NdBits B;
  const uintptr_t addr = (uintptr_t) data + first_byte;
  B.wbase = (const uint32_t *) (addr & ~(uintptr_t) 3);
  B.first = (uint32_t) (addr & 3);
  B.end = B.first + bytes;
  return B;
}

// word w as the big-endian value of its bytes; bytes at and past the end read as 0xff (guard bit 1)
__device__ __forceinline__ uint32_t
nd_word (const NdBits & B, uint32_t w)
{
  const uint32_t b0 = 4u * w;
  if (b0 >= B.end)
    return 0xffffffffu;
  uint32_t v = __builtin_bswap32 (gload < uint32_t > (B.wbase + w));
  if (b0 + 4u > B.end)
    v |= 0xffffffffu >> (8u * (B.end - b0));
  return v;
}

// the 64 bits from bit `pos` on
__device__ __forceinline__ uint64_t
nd_bits64 (const NdBits & B, uint64_t pos)
{
  const uint64_t at = 8ull * B.first + pos;
  if (at >= 8ull * B.end)
    return ~0ull;
  const uint32_t w = (uint32_t) (at >> 5), sh = (uint32_t) at & 31u;
  const uint32_t a = nd_word (B, w), b = nd_word (B, w + 1), c = nd_word (B, w + 2);
  const uint64_t hi = ((uint64_t) a << 32) | b;
  return sh ? (hi << sh) | (c >> (32u - sh)) : hi;
}

// a bit position as a record's word (positions behind 2^32 lie behind every chunk)
__device__ __forceinline__ uint32_t
nd_sat32 (uint64_t pos)
{
  return pos > 0xffffffffull ? 0xffffffffu : (uint32_t) pos;
}

// bit 2 i of x to bit i
__device__ __forceinline__ uint32_t
nd_compress (uint64_t x)
{
  x &= 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
  x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
  x = (x | (x >> 16)) & 0x00000000ffffffffull;
  return (uint32_t) x;
}

// One code at bit `pos` (schro_unpack_decode_uint / _sint as schro_hip.h defines them past count 30): the value as 32 bits,
// pos moved behind it.  The loop runs once per 32 data bits: never for a code an encoder writes, and to the end of the
// bytes at most, where every bit reads 1.
__device__ __forceinline__ uint32_t
nd_code (const NdBits & B, uint64_t & pos, uint32_t & longs, bool is_signed)
{
  uint64_t w = nd_bits64 (B, pos);
  if (w >> 63) {
    pos += 1;
    return 0;
  }
  uint64_t x = w & kFollow;
  uint32_t v = 1, n = 0;
#pragma unroll 1
  while (x == 0) {
    v = nd_compress (w);        // (v << 32 | 32 data bits) mod 2^32
    n = min (n + 32u, 1u << 30);
    pos += 64;
    w = nd_bits64 (B, pos);
    x = w & kFollow;
  }
  const uint32_t k = (uint32_t) __clzll ((long long) x) >> 1;   // pairs in front of the follow 1: 0 .. 31
  if (k)
    v = (v << k) | nd_compress (w >> (64u - 2u * k));
  n += k;
  pos += 2u * k + 1u;
  uint32_t m = v - 1u;
  if (is_signed) {
    if ((w >> (62u - 2u * k)) & 1u)
      m = 0u - m;
    pos += 1;
  }
  longs += n >= 31u ? 1u : 0u;
  return m;
}

// ---- the state machine over one chunk ----------------------------------------------------------------------------------

struct NdWalk {
  uint32_t off, state, count;
};

// from bit `off` of w in `state`, until `limit` codes have completed or the chunk ends
__device__ __forceinline__ NdWalk
nd_walk (uint64_t w, uint32_t off, uint32_t state, uint32_t limit)
{
  NdWalk r;
  uint32_t count = 0;
#pragma unroll 1
  while (count < limit && off < 64u) {
    if (state == kD) {
      off += 1;
      state = kF;
    } else if (state == kS) {
      off += 1;
      state = kA;
      count += 1;
    } else if (state == kA) {
      // a run of 1-bits: that many codes of value 0
      const uint64_t x = ~(w << off);
      const uint32_t ones = x ? (uint32_t) __clzll ((long long) x) : 64u;
      const uint32_t z = min (min (ones, 64u - off), limit - count);
      count += z;
      off += z;
      if (z < ones || count >= limit || off >= 64u)
        continue;               // (z == ones < what was asked for: the bit at `off` is 0)
      state = kF;               // a 0 at a code's start is a follow 0
    } else {
      // (follow, data) pairs up to the follow 1
      const uint64_t x = (w << off) & kFollow;
      if (x == 0) {
        state = ((64u - off) & 1u) ? kD : kF;
        off = 64u;
      } else {
        off += (uint32_t) __clzll ((long long) x) + 1u;
        state = kS;
      }
    }
  }
  r.off = off;
  r.state = state;
  r.count = count;
  return r;
}

__device__ __forceinline__ uint32_t
nd_pick (const uint32_t f[4], uint32_t s)
{
  return s == 0 ? f[0] : s == 1 ? f[1] : s == 2 ? f[2] : f[3];
}

// maps of the four states, each completions << 2 | exit state: `then` behind `first`
__device__ __forceinline__ void
nd_compose (uint32_t out[4], const uint32_t first[4], const uint32_t then[4])
{
#pragma unroll
  for (int s = 0; s < 4; s++)
    out[s] = (first[s] & ~3u) + nd_pick (then, first[s] & 3u);
}

}                               // namespace
}                               // namespace schro
