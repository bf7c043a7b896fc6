// unpack_fetch.h -- one sample of a packed picture (or of a planar plane) on the device: what unpack.hip's kernel and
// the packed fetch stage of iwt_fwd.hip's level 0 share.
//
// The source side of schro_virt_frame_new_unpack (schrovirtframe.c:616-940) per sample: where the sample's bits lie in
// its row, and what they are worth in the unpacked frame's own depth (u8 for YUYV / UYVY / AYUV, s16 for v210 / v216,
// s32 for AY64; a planar plane: itself).  A row is read in 16-byte words; consecutive samples of a lane mostly share a
// word, so the word last loaded is kept (RowWords).  A sample whose word would reach past the row's last byte is read
// alone, with a load of its own size: nothing outside [row, row + row_bytes) is ever touched.
#pragma once

#include "schro_hip_internal.h"

namespace schro {

#ifdef __HIPCC__
typedef uint16_t u16_u __attribute__ ((aligned (1)));

// the word of a row a lane loaded last
struct RowWords {
  const uint8_t *row;
  int q;                        // index of the 16-byte word in `w`, -1: none
  u32x4 w;
};

// the `nb` bytes (1, 2 or 4; b % nb == 0) at byte b of the row, little endian, in the low bits
__device__ __forceinline__ uint32_t
row_bits (RowWords & rw, const uint8_t * row, int row_bytes, int b, int nb)
{
  const int q = b >> 4;
  if (16 * q + 16 <= row_bytes) {
    if (row != rw.row || q != rw.q) {
      rw.w = gload < u32x4_u > (row + 16 * q);
      rw.row = row;
      rw.q = q;
    }
    const int k = (b >> 2) & 3;
    const uint32_t d = k == 0 ? rw.w.x : k == 1 ? rw.w.y : k == 2 ? rw.w.z : rw.w.w;
    return d >> (8 * (b & 3));
  }
  if (nb == 1)
    return gload < uint8_t > (row + b);
  if (nb == 2)
    return gload < u16_u > (row + b);
  return gload < u32_u > (row + b);
}

// v210 (schrovirtframe.c:765-863): six pixels in four words; sample x of component `comp` lies in word 4 * g + word_of,
// at bit 10 * tenth_of.  The divisions are by constants.
__device__ __forceinline__ void
v210_place (int comp, int x, int *word, int *shift)
{
  if (comp == 0) {
    const int g = x / 6, r = x - 6 * g;
    *word = 4 * g + ((0xf94 >> (2 * r)) & 3);   // 0, 1, 1, 2, 3, 3
    *shift = 10 * ((0x861 >> (2 * r)) & 3);     // 10, 0, 20, 10, 0, 20
  } else {
    const int g = x / 3, r = x - 3 * g;
    *word = 4 * g + (((comp == 1 ? 0x24 : 0x38) >> (2 * r)) & 3);       // U: 0, 1, 2; V: 0, 2, 3
    *shift = 10 * (((comp == 1 ? 0x24 : 0x12) >> (2 * r)) & 3); // U: 0, 10, 20; V: 20, 0, 10
  }
}

// sample x of a row, in the unpacked frame's own depth; KIND = s.kind
template < int KIND >
__device__ __forceinline__ int
unpack_sample (RowWords & rw, const UnpackSrc & s, const uint8_t * row, int x)
{
  if constexpr (KIND == kUnpackV210) {
    int word, shift;
    v210_place (s.comp, x, &word, &shift);
    return (int) ((row_bits (rw, row, s.row_bytes, 4 * word, 4) >> shift) & 0x3ff) - 512;
  } else if constexpr (KIND == kUnpackU16) {    // AY64: word - 32768
    return (int) (row_bits (rw, row, s.row_bytes, x * s.xmul + s.xoff, 2) & 0xffff) - 32768;
  } else if constexpr (KIND == kUnpackS16) {
    return (int16_t) row_bits (rw, row, s.row_bytes, x * s.xmul + s.xoff, 2);
  } else if constexpr (KIND == kUnpackS32) {
    return (int) row_bits (rw, row, s.row_bytes, x * s.xmul + s.xoff, 4);
  } else {                      // kUnpackU8: a byte (v216: the HIGH byte of its word, no offset, schrovirtframe.c:876-888)
    return (int) (row_bits (rw, row, s.row_bytes, x * s.xmul + s.xoff, 1) & 0xff);
  }
}

// The source kind is uniform per workgroup: one scalar switch in front of a lane's loop over its samples, f (kind as a
// compile-time constant) -- each loop body holds one kind's extraction and unrolls.
template < int KIND > struct UnpackKind {
  static constexpr int value = KIND;
};
template < typename F >
__device__ __forceinline__ void
unpack_by_kind (int kind, F && f)
{
  switch (kind) {
    case kUnpackV210: f (UnpackKind < kUnpackV210 > ()); break;
    case kUnpackU16: f (UnpackKind < kUnpackU16 > ()); break;
    case kUnpackS16: f (UnpackKind < kUnpackS16 > ()); break;
    case kUnpackS32: f (UnpackKind < kUnpackS32 > ()); break;
    default: f (UnpackKind < kUnpackU8 > ()); break;
  }
}

// the depth step of schro_frame_convert (schroframe.c:905-924) from `from` to `to` bytes per sample (1: u8):
// orc_offsetconvert_s16_u8 / _s32_u8 (x - 128), orc_convert_s32_s16 (sign extension), orc_convert_s16_s32 (truncation: the
// store's), orc_offsetconvert_u8_s16 (16-bit wrapping + 128, then 0 .. 255), orc_offsetconvert_u8_s32 (32-bit wrapping
// + 128, saturated to s16, then 0 .. 255)
__device__ __forceinline__ int
unpack_depth (int v, int from, int to)
{
  if (from == to)
    return v;
  if (from == 1)
    return v - 128;
  if (to == 1) {
    const int t = from == 2 ? (int) (int16_t) (v + 128) : (int) ((uint32_t) v + 128u);
    return min (max (t, 0), 255);
  }
  return v;
}
#endif

}                               // namespace schro
