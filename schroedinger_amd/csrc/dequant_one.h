// dequant_one.h -- the quantiser tables and the reconstruction of one value, shared by dequant.hip (values handed over by
// a host entropy decoder) and noarith_dec.hip (values read from the VLC stream on the device).
#pragma once

#include "schro_hip_internal.h"

namespace schro {
namespace {

struct QuantTables3 {
  uint32_t factor[61], off12[61], off38[61];
};
constexpr QuantTables3
make_quant_tables3 ()
{
  QuantTables3 t = { };
  for (int q = 0; q <= 60; q++) {
    // Dirac specification 13.3.1; all 61 entries of each table are pinned against the
    // reference's numbers by tests (quant_tables.json, arith_lut.json)
    const uint64_t base = (uint64_t) 1 << (q / 4);
    const uint64_t f = (q & 3) == 0 ? 4 * base : (q & 3) == 1 ? (503829 * base + 52958) / 105917
        : (q & 3) == 2 ? (665857 * base + 58854) / 117708 : (440253 * base + 32722) / 65444;
    t.factor[q] = (uint32_t) f;
    t.off12[q] = q == 0 ? 1u : q == 1 ? 2u : (uint32_t) ((f + 1) / 2);
    t.off38[q] = q == 0 ? 1u : (uint32_t) ((f * 3 + 4) / 8);
  }
  return t;
}
constexpr QuantTables3 kHostQuant = make_quant_tables3 ();
static __device__ __constant__ QuantTables3 kDevQuant = make_quant_tables3 ();     // (plans: the kernel looks the quantiser up)

template < typename T, int ARITH >
__device__ __forceinline__ T
dequant_one (int32_t q, uint32_t factor, uint32_t offset)
{
  if constexpr (ARITH == 1) {
    const int16_t qs = (int16_t) q;
    const int16_t sign = qs > 0 ? 1 : (qs < 0 ? -1 : 0);
    const int16_t mag = (int16_t) (qs < 0 ? -qs : qs);          // absw: -32768 stays -32768
    int16_t t = (int16_t) (mag * (int16_t) factor);
    t = (int16_t) (t + (int16_t) (offset + 2u));
    t = (int16_t) (t >> 2);
    return (T) (int16_t) (t * sign);
  } else {
    if (q == 0)
      return (T) 0;
    const uint32_t mag = q < 0 ? 0u - (uint32_t) q : (uint32_t) q;
    const int32_t d = (int32_t) (mag * factor + offset + 2u) >> 2;
    return (T) (q < 0 ? (int32_t) (0u - (uint32_t) d) : d);
  }
}

}                               // namespace
}                               // namespace schro
