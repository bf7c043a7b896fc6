// motion_arith_dec.hip -- the motion data of an arithmetic-coded picture, read on the device: the twin of
// schro_decoder_parse_block_data and schro_decoder_decode_block_data / _decode_macroblock / _decode_prediction_unit
// (schrodecoder.c:2531-2814) for !params->is_noarith, over the predictors of schromotion.c:163-430 and the binary
// arithmetic decoder of arith_bin.h.  schro_hip.h states the rules.
//
// The nine sections are nine independent coders, and no bin's context depends on a decoded neighbour: a split is a uint
// over SB_F1 -> SB_F2 -> SB_F2 .., SB_DATA; a mode bit one bin in BLOCK_MODE_REF1 / _REF2; a vector or DC residual a sint
// over the section's fixed chain of continuation contexts, VALUE and SIGN, its loop stopped after 30 data bins.  So a
// section's k-th value is the same whatever the field is; only how many values a section is asked for depends on the field.
// motion_dec.hip's two facts carry over: any order that respects x + y computes the field, and a unit's index in a section
// is a prefix count in stream order.  A code's start cannot be found without decoding what precedes it, so there are no
// chunk summaries, no scan and no extract: a section is one serial chain of bins, and the walks run between the chains.
//
//   ma_header_kernel   thread 0 of a wave per picture walks the 7 or 9 headers as md_header_kernel does and writes every
//                      word of the result.
//   ma_chain_kernel    a wave per chain, lane 0 deciding ONE BIN PER TRIP of its loop.  Launched three times: the splits
//                      (section 0: x * y / 16 uints), the modes (section 1 without global motion: units * (1 + (num_refs >
//                      1)) bins, stored per unit) and the values (sections 2 .. 8, a wave each: section_units sints, stored
//                      as 32-bit residuals by index).  At most seven probabilities and the 256-entry table sit in LDS, and
//                      so does the input: the wave's 64 lanes fetch a window of 64 aligned dwords, lane 0 decides until
//                      the two bytes its next bin may take lie behind the window, and the wave fetches again.  The
//                      dependent path of a bin is then arithmetic and LDS reads.
//   ma_split_kernel    md_split_kernel: splits over anti-diagonals of superblocks, then the prefix sum of 1, 4 or 16.
//   ma_mode_kernel     md_mode_kernel: modes over anti-diagonals of blocks from the unit's stored bins.  With global motion
//                      a unit's third bin (GLOBAL_BLOCK) exists only when its mode is not 0: thread 0 walks the units in
//                      stream order, predicting and decoding together (correct and slow).  Then the three prefix counts.
//   ma_value_kernel    md_value_kernel: vectors and DCs over anti-diagonals of blocks, residuals by index, whole 20-byte
//                      records for every block of the unit; then the masks from the coders' offsets.
//
// No store leaves `motion`, `result` and the scratch; input bytes are fetched as the aligned words that hold them.  No
// loop has a cap of its own: DESIGN 4.25 gives the bound that follows from the input.

#include "motion_common.h"
#include "na_chunks.h"
#include "arith_bin.h"
#include "motion_walks.h"

namespace schro {
namespace {

enum { kMaFirst = 0, kMaBytes, kMaLength, kMaUnits };
static_assert (kMaUnits + 1 == kMaSecWords, "the words of a section");

// Dirac specification, the arithmetic decoder's probability update table (256 entries): arith_dec.hip's kAdLut stated again
// (a __constant__ array belongs to one file); pinned against it and against the reference's numbers
// (tests/golden/arith_lut.json) by tests/test_motion_arith_dec_ref.py
static __device__ __constant__ uint16_t kMaLut[256] = {
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

constexpr int kMaWindow = 64;   // dwords of input a wave keeps in LDS: a dword per lane

struct MaScratch {
  uint32_t *sec, *res0, *split, *unit_first, *mode, *res, *st, *idx;
  uint32_t nsb, blocks;
};

__device__ __forceinline__ MaScratch
ma_scratch (const MaPicture & pic, uint32_t * scratch)
{
  MaScratch S;
  S.blocks = (uint32_t) pic.nbx * (uint32_t) pic.nby;
  S.nsb = S.blocks >> 4;
  S.sec = scratch + pic.scratch_first;
  S.res0 = S.sec + kMdSections * kMaSecWords;
  S.split = S.res0 + S.nsb;
  S.unit_first = S.split + S.nsb;
  S.mode = S.res0 + ((3 * (size_t) S.nsb + 1) & ~(size_t) 1);
  S.res = S.mode + S.blocks;
  S.st = S.res + 7 * (size_t) S.blocks;
  S.idx = S.st + S.blocks;
  return S;
}

__device__ __forceinline__ bool
ma_absent (const MaPicture & pic, int s)
{
  return pic.num_refs < 2 && (s == 4 || s == 5);
}

__device__ __forceinline__ NdBits
ma_section_bits (const MaPicture & pic, const uint32_t * sec)
{
  return nd_bits (pic.data, gload < uint32_t > (sec + kMaFirst), gload < uint32_t > (sec + kMaBytes));
}

__device__ __forceinline__ uint32_t
ma_sat32 (uint64_t v)
{
  return v > 0xffffffffull ? 0xffffffffu : (uint32_t) v;
}

// ---- header ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (64)
void ma_header_kernel (const MaPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  if (threadIdx.x != 0)
    return;
  const MaPicture & pic = pics[blockIdx.x];
  const MaScratch S = ma_scratch (pic, scratch);
  SchroHipMotionArithDecodeResult *res = pic.result;
  uint32_t L = pic.data_bytes;
  if (pic.bytes_on_device)
    L = min (L, gload < uint32_t > (pic.bytes_on_device));
  const NdBits O = nd_bits (pic.data, 0, L);
  uint64_t pos = 0;
  uint32_t longs = 0, truncated = 0;
#pragma unroll 1
  for (int s = 0; s < kMdSections; s++) {
    uint32_t first = 0, bytes = 0, length = 0;
    const bool absent = ma_absent (pic, s);
    if (!absent) {
      pos = (pos + 7u) & ~7ull;
      length = nd_code (O, pos, longs, false);
      pos = (pos + 7u) & ~7ull;
      const uint64_t fb = pos >> 3;
      bytes = fb < L ? min (length, L - (uint32_t) fb) : 0u;
      truncated |= (bytes < length ? 1u : 0u) << s;
      pos += 8ull * length;
      first = bytes ? (uint32_t) fb : 0u;
    }
    uint32_t *sec = S.sec + s * kMaSecWords;
    gstore < uint32_t > (sec + kMaFirst, first);
    gstore < uint32_t > (sec + kMaBytes, bytes);
    gstore < uint32_t > (sec + kMaLength, length);
    gstore < uint32_t > (sec + kMaUnits, 0u);
    gstore < uint32_t > (&res->section_bytes[s], bytes);
    gstore < uint32_t > (&res->section_units[s], 0u);
    gstore < uint32_t > (&res->section_offset[s], absent ? 0u : 3u);
    gstore < uint32_t > (&res->section_bins[s], 0u);
  }
  const uint64_t behind = (pos + 7u) >> 3;
  gstore < uint32_t > (&res->bytes, behind < L ? (uint32_t) behind : L);
  gstore < uint32_t > (&res->truncated, truncated);
  gstore < uint32_t > (&res->overran, 0u);
  gstore < uint32_t > (&res->not_consumed, 0u);
  gstore < uint32_t > (&res->long_codes, longs);
  gstore < uint32_t > (&res->unverified, 0u);
  gstore < int32_t > (&res->first_unverified, -1);
}

// ---- the chains ----------------------------------------------------------------------------------------------------------

// a payload seen through the wave's window: dwords w0 .. w0 + kMaWindow - 1 from the payload's aligned base, each as the
// big-endian value of its bytes
struct MaWindow {
  const uint32_t *win;
  uint32_t w0;
  uint32_t first, end;          // NdBits' bytes
};

// byte `off` of the payload; 0xff behind its end.  The caller keeps the bytes it asks for inside the window.
__device__ __forceinline__ uint32_t
ad_byte (const MaWindow & W, uint32_t off)
{
  const uint32_t at = W.first + off;
  if (at >= W.end)
    return 0xffu;
  return (W.win[(at >> 2) - W.w0] >> (24u - 8u * (at & 3u))) & 0xffu;
}

// what the bin a lane decides next is
enum { kStCont, kStValue, kStSign, kStMode };

// phase 0: section 0; phase 1: section 1 (without global motion); phase 2: section 2 + blockIdx.x
__global__ __launch_bounds__ (64)
void ma_chain_kernel (const MaPicture * __restrict__ pics, uint32_t * __restrict__ scratch, int phase)
{
  __shared__ uint32_t win[kMaWindow];
  __shared__ uint16_t prob[8];
  __shared__ uint16_t lut[256];
  __shared__ uint32_t next[2];  // whether the chain goes on, and from which dword
  const int lane = (int) threadIdx.x;
  const MaPicture & pic = pics[blockIdx.y];
  const MaScratch S = ma_scratch (pic, scratch);
  const int s = phase == 2 ? 2 + (int) blockIdx.x : phase;
  if (ma_absent (pic, s) || (phase == 1 && pic.have_global))
    return;
  const uint32_t *sec = S.sec + s * kMaSecWords;
  // the values the chain owes: every superblock's split, every unit's mode bins, the units that select the section
  const uint32_t n = phase == 0 ? S.nsb : gload < uint32_t > (sec + kMaUnits);
  if (n == 0)
    return;                     // (offset 3, no bins: the header launch has said so)
  const NdBits B = ma_section_bits (pic, sec);
  for (int k = lane; k < 256; k += 64)
    lut[k] = kMaLut[k];
  if (lane < 8)
    prob[lane] = 0x8000u;

  // the contexts of the chain, as indices into prob: continuation bins 0 .. ncont - 1 (the last repeats), then the data
  // bins' and the sign's; the modes' are REF1, REF2
  const uint32_t ncont = phase == 0 ? 2u : s < 6 ? 5u : 2u;
  const uint32_t mode_bins = pic.num_refs > 1 ? 2u : 1u;
  uint32_t *out = phase == 0 ? S.res0 : phase == 1 ? S.mode : S.res + (size_t) (s - 2) * S.blocks;

  MaWindow W = { win, 0u, B.first, B.end };
  AdCoder a = { 0xffff0000u, 0u, 3u, 16u };
  uint32_t k = 0, stage = phase == 1 ? kStMode : kStCont, bits = 1, count = 0, unit = 0, longs = 0;
  uint64_t bins = 0;
  bool fresh = true;
  uint32_t w0 = 0;
#pragma unroll 1
  for (;;) {
    // the window: a dword per lane, of those that hold at least one byte of the payload
    const uint32_t w = w0 + (uint32_t) lane;
    win[lane] = 4u * w < B.end ? __builtin_bswap32 (gload < uint32_t > (B.wbase + w)) : 0xffffffffu;
    __syncthreads ();
    if (lane == 0) {
      W.w0 = w0;
      if (fresh) {
        ad_init (a, W);         // (bytes 0 .. 3 of the payload: dwords 0 and 1 at the most)
        fresh = false;
      }
      uint32_t go = 0;
#pragma unroll 1
      while (k < n) {
        // a bin takes at most the two bytes behind `offset`: those of them inside the payload must lie in the window
        const uint32_t lo = B.first + a.offset + 1u;
        if (lo < B.end && (min (lo + 1u, B.end - 1u) >> 2) >= w0 + (uint32_t) kMaWindow) {
          go = 1;
          w0 = lo >> 2;
          break;
        }
        const uint32_t ctx = stage == kStCont ? min (count, ncont - 1u) : stage == kStValue ? ncont : stage == kStSign ? ncont + 1u : count;
        const uint32_t bit = ad_bin (a, W, &prob[ctx], lut);
        bins++;
        bool done = false;
        uint32_t value = 0;
        if (stage == kStMode) {
          // a unit's bins: bit 0 ref-1, bit 1 ref-2
          unit |= bit << count;
          if (++count == mode_bins) {
            value = unit;
            unit = 0;
            done = true;
          }
        } else if (stage == kStCont) {
          if (!bit) {
            stage = kStValue;
          } else {
            longs += count >= 31u;
            value = bits - 1u;
            if (phase == 2 && value)
              stage = kStSign;
            else
              done = true;
          }
        } else if (stage == kStValue) {
          bits = (bits << 1) | bit;
          count = min (count + 1u, 31u);
          stage = kStCont;
          if (phase == 2 && count == 30u)
            stage = kStSign;    // (30 data bins: bits - 1 is not 0)
        } else {
          value = bit ? 0u - (bits - 1u) : bits - 1u;
          done = true;
        }
        if (done) {
          gstore < uint32_t > (out + k, value);
          k++;
          bits = 1;
          count = 0;
          stage = phase == 1 ? kStMode : kStCont;
        }
      }
      next[0] = go;
      next[1] = w0;
    }
    __syncthreads ();
    const uint32_t go = next[0];
    w0 = next[1];
    __syncthreads ();
    if (!go)
      break;
  }
  if (lane == 0) {
    SchroHipMotionArithDecodeResult *res = pic.result;
    gstore < uint32_t > (&res->section_offset[s], a.offset);
    gstore < uint32_t > (&res->section_bins[s], ma_sat32 (bins));
    if (longs)                  // (section 0 alone, behind the header launch: one writer)
      gstore < uint32_t > (&res->long_codes, gload < uint32_t > (&res->long_codes) + longs);
  }
}

// ---- the walks -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (kMdSplitThreads)
void ma_split_kernel (const MaPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  __shared__ uint32_t part[kMdSplitThreads];
  const MaPicture & pic = pics[blockIdx.x];
  const MaScratch S = ma_scratch (pic, scratch);
  const int nsbx = pic.nbx >> 2, nsby = pic.nby >> 2, nsb = (int) S.nsb;
  const int tid = (int) threadIdx.x, T = kMdSplitThreads;
  // schro_motion_split_prediction (schromotion.c:371-399) and the residual
  walk_diagonals (nsbx, nsby, tid, T, [&](int x, int y) {
      const int k = y * nsbx + x;
      uint32_t pred = 0;
      if (y == 0) {
        if (x > 0)
          pred = gload < uint32_t > (S.split + k - 1);
      } else if (x == 0) {
        pred = gload < uint32_t > (S.split + k - nsbx);
      } else {
        pred = (gload < uint32_t > (S.split + k - nsbx) + gload < uint32_t > (S.split + k - 1) + gload < uint32_t > (S.split + k - nsbx - 1) + 1u) / 3u;
      }
      gstore < uint32_t > (S.split + k, (uint32_t) (((uint64_t) pred + gload < uint32_t > (S.res0 + k)) % 3u));
  });
  // every superblock's first unit: the prefix sum of 1, 4 or 16, a run of superblocks per thread
  const int run = (nsb + T - 1) / T;
  const int c0 = min (nsb, tid * run), c1 = min (nsb, c0 + run);
  uint32_t mine[1] = { 0u };
  for (int c = c0; c < c1; c++)
    mine[0] += 1u << (2u * gload < uint32_t > (S.split + c));
  md_block_scan < 1 > (part, mine);
  uint32_t at = part[tid] - mine[0];
  for (int c = c0; c < c1; c++) {
    gstore < uint32_t > (S.unit_first + c, at);
    at += 1u << (2u * gload < uint32_t > (S.split + c));
  }
  if (tid == T - 1) {
    gstore < uint32_t > (S.sec + 0 * kMaSecWords + kMaUnits, S.nsb);
    gstore < uint32_t > (S.sec + 1 * kMaSecWords + kMaUnits, part[tid]);
    gstore < uint32_t > (&pic.result->section_units[0], S.nsb);
    gstore < uint32_t > (&pic.result->section_units[1], part[tid]);
  }
}

__global__ __launch_bounds__ (kMdWalkThreads)
void ma_mode_kernel (const MaPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  __shared__ uint32_t part[3 * kMdWalkThreads];
  const MaPicture & pic = pics[blockIdx.x];
  const MaScratch S = ma_scratch (pic, scratch);
  const int nbx = pic.nbx, nsbx = nbx >> 2, nsb = (int) S.nsb;
  const int tid = (int) threadIdx.x, T = kMdWalkThreads;
  if (!pic.have_global) {
    walk_diagonals (nbx, pic.nby, tid, T, [&](int x, int y) {
        const int sb = (y >> 2) * nsbx + (x >> 2);
        const uint32_t split = gload < uint32_t > (S.split + sb);
        const int step = 4 >> split;
        if ((x | y) & (step - 1))
          return;               // not a unit's origin
        const uint32_t n = gload < uint32_t > (S.unit_first + sb) + ((((uint32_t) y & 3u) >> (2u - split)) << split) + (((uint32_t) x & 3u) >> (2u - split));
        const uint32_t r = gload < uint32_t > (S.mode + n);
        const uint32_t mode = (md_majority (S.st, nbx, x, y) ^ r) & 3u;
        md_store_unit (S.st, nbx, x, y, step, mode | (split << 3));
    });
  } else {
    if (tid == 0) {
      // the section's coder, in step with the predictions: REF1, REF2 and GLOBAL_BLOCK
      const NdBits B = ma_section_bits (pic, S.sec + 1 * kMaSecWords);
      AdCoder a;
      ad_init (a, B);
      uint32_t p1 = 0x8000u, p2 = 0x8000u, pg = 0x8000u;
      uint64_t bins = 0;
#pragma unroll 1
      for (int sb = 0; sb < nsb; sb++) {
        const uint32_t split = gload < uint32_t > (S.split + sb);
        md_units (nsbx, sb, split, [&](int x, int y) {
            const uint32_t maj = md_majority (S.st, nbx, x, y);
            uint32_t r = ad_bin (a, B, &p1, kMaLut);
            bins++;
            if (pic.num_refs > 1) {
              r |= ad_bin (a, B, &p2, kMaLut) << 1;
              bins++;
            }
            const uint32_t mode = (maj ^ r) & 3u;
            uint32_t ug = 0;
            if (mode) {
              ug = ((maj >> 2) ^ ad_bin (a, B, &pg, kMaLut)) & 1u;
              bins++;
            }
            md_store_unit (S.st, nbx, x, y, 4 >> split, mode | (ug << 2) | (split << 3));
        });
      }
      gstore < uint32_t > (&pic.result->section_offset[1], a.offset);
      gstore < uint32_t > (&pic.result->section_bins[1], ma_sat32 (bins));
    }
    __syncthreads ();
  }

  // which value of its sections a unit owns: the counts, in stream order, of the units before it that select ref-1, ref-2
  // and the DCs -- a run of superblocks per thread
  const int run = (nsb + T - 1) / T;
  const int c0 = min (nsb, tid * run), c1 = min (nsb, c0 + run);
  uint32_t mine[3] = { 0u, 0u, 0u };
  for (int sb = c0; sb < c1; sb++)
    md_units (nsbx, sb, gload < uint32_t > (S.split + sb), [&](int x, int y) {
        const uint32_t f = gload < uint32_t > (S.st + (size_t) y * nbx + x);
        mine[0] += (f & 1u) && !(f & 4u);
        mine[1] += (f & 2u) && !(f & 4u);
        mine[2] += (f & 3u) == 0u;
    });
  md_block_scan < 3 > (part, mine);
  uint32_t at[3];
#pragma unroll
  for (int k = 0; k < 3; k++)
    at[k] = part[k * T + tid] - mine[k];
  for (int sb = c0; sb < c1; sb++)
    md_units (nsbx, sb, gload < uint32_t > (S.split + sb), [&](int x, int y) {
        const size_t k = (size_t) y * nbx + x;
        const uint32_t f = gload < uint32_t > (S.st + k);
        gstore < uint32_t > (S.idx + 2 * k, (f & 3u) == 0u ? at[2] : at[0]);
        gstore < uint32_t > (S.idx + 2 * k + 1, at[1]);
        at[0] += (f & 1u) && !(f & 4u);
        at[1] += (f & 2u) && !(f & 4u);
        at[2] += (f & 3u) == 0u;
    });
  if (tid == T - 1) {
    for (int s = 2; s < kMdSections; s++) {
      const uint32_t units = ma_absent (pic, s) ? 0u : part[(s < 4 ? 0 : s < 6 ? 1 : 2) * T + tid];
      gstore < uint32_t > (S.sec + s * kMaSecWords + kMaUnits, units);
      gstore < uint32_t > (&pic.result->section_units[s], units);
    }
  }
}

__global__ __launch_bounds__ (kMdWalkThreads)
void ma_value_kernel (const MaPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  __shared__ uint32_t tot_unverified, tot_first, overran, not_consumed;
  const MaPicture & pic = pics[blockIdx.x];
  const MaScratch S = ma_scratch (pic, scratch);
  const int nbx = pic.nbx;
  const int tid = (int) threadIdx.x, T = kMdWalkThreads;
  uint8_t *field = pic.motion;
  if (tid == 0)
    tot_unverified = 0, tot_first = 0xffffffffu, overran = 0, not_consumed = 0;
  uint32_t unverified = 0, first = 0xffffffffu;
  walk_diagonals (nbx, pic.nby, tid, T, [&](int x, int y) {
      const size_t k = (size_t) y * nbx + x;
      const uint32_t flags = gload < uint32_t > (S.st + k);
      const int step = 4 >> (flags >> 3);
      if ((x | y) & (step - 1))
        return;                 // not a unit's origin
      const uint32_t mode = flags & 3u;
      const uint32_t ia = gload < uint32_t > (S.idx + 2 * k), ib = gload < uint32_t > (S.idx + 2 * k + 1);
      MdNeighbours nb;
      nb.x = x, nb.y = y;
      nb.left = nb.above = nb.diag = MdRec { 0u, 0u, 0u };
      if (x > 0)
        nb.left = md_load (field, nbx, x - 1, y);
      if (y > 0)
        nb.above = md_load (field, nbx, x, y - 1);
      if (x > 0 && y > 0)
        nb.diag = md_load (field, nbx, x - 1, y - 1);
      uint32_t dxw = 0, dyw = 0;
      if (mode == 0) {
        // schro_motion_dc_prediction (:163-210): the neighbours of mode 0, whatever their global flag
        const bool pl = x > 0 && (nb.left.flags & 3u) == 0, pa = y > 0 && (nb.above.flags & 3u) == 0;
        const bool pd = x > 0 && y > 0 && (nb.diag.flags & 3u) == 0;
        const int n = (int) pl + (int) pa + (int) pd;
        bool bad = false;
        uint32_t dc[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const int sum = (pl ? md_dc (nb.left, i) : 0) + (pa ? md_dc (nb.above, i) : 0) + (pd ? md_dc (nb.diag, i) : 0);
          const int pred = n == 0 ? 0 : n == 1 ? (int) (int16_t) sum : n == 2 ? (sum + 1) >> 1 : ((sum + 1) * 21845 + 10922) >> 16;
          const uint32_t r = gload < uint32_t > (S.res + (size_t) (4 + i) * S.blocks + ia);
          const int v = (int16_t) ((uint32_t) pred + r);
          bad |= v < -128 || v > 127;
          dc[i] = (uint32_t) v & 0xffffu;
        }
        dxw = dc[0] | (dc[1] << 16);
        dyw = dc[2];
        if (bad) {
          unverified += (uint32_t) (step * step);
          first = min (first, (uint32_t) k);
        }
      } else if (!(flags & 4u)) {
#pragma unroll
        for (int ref = 0; ref < 2; ref++)
          if (mode & (1u << ref)) {
            int px, py;
            vector_prediction (nb, x, y, 1 << ref, &px, &py);
            const uint32_t i = ref ? ib : ia;
            const uint32_t rx = gload < uint32_t > (S.res + (size_t) (2 * ref) * S.blocks + i);
            const uint32_t ry = gload < uint32_t > (S.res + (size_t) (2 * ref + 1) * S.blocks + i);
            dxw |= (((uint32_t) px + rx) & 0xffffu) << (16 * ref);
            dyw |= (((uint32_t) py + ry) & 0xffffu) << (16 * ref);
          }
      }
      for (int l = 0; l < step; l++)
        for (int c = 0; c < step; c++) {
          uint8_t *mv = mv_record (field, nbx, x + c, y + l);
          gstore < uint32_t > (mv + kMvFlags, flags);
          gstore < uint32_t > (mv + kMvMetric, 0u);
          gstore < uint32_t > (mv + kMvChromaMetric, 0u);
          gstore < uint32_t > (mv + kMvDx, dxw);
          gstore < uint32_t > (mv + kMvDy, dyw);
        }
  });
  if (unverified) {
    atomicAdd (&tot_unverified, unverified);
    atomicMin (&tot_first, first);
  }
  // where each coder stands against its stated length (schrodecoder.c:2594, :2598)
  if (tid < kMdSections && !ma_absent (pic, tid)) {
    const uint64_t offset = gload < uint32_t > (&pic.result->section_offset[tid]);
    const uint64_t length = gload < uint32_t > (S.sec + tid * kMaSecWords + kMaLength);
    if (offset > length + 6u)
      atomicOr (&overran, 1u << tid);
    if (offset < length)
      atomicOr (&not_consumed, 1u << tid);
  }
  __syncthreads ();
  if (tid == 0) {
    gstore < uint32_t > (&pic.result->overran, overran);
    gstore < uint32_t > (&pic.result->not_consumed, not_consumed);
    gstore < uint32_t > (&pic.result->unverified, tot_unverified);
    gstore < int32_t > (&pic.result->first_unverified, tot_unverified ? (int32_t) tot_first : -1);
  }
}

}                               // namespace

int
launch_motion_arith_decode (hipStream_t stream, const MaPicture * d_pics, int npics, uint32_t * scratch, int stages)
{
  if (stages & 1)
    SCHRO_LAUNCH (ma_header_kernel, dim3 (npics), dim3 (64), 0, stream, d_pics, scratch);
  if (stages & 2)
    SCHRO_LAUNCH (ma_chain_kernel, dim3 (1, npics), dim3 (64), 0, stream, d_pics, scratch, 0);
  if (stages & 4)
    SCHRO_LAUNCH (ma_split_kernel, dim3 (npics), dim3 (kMdSplitThreads), 0, stream, d_pics, scratch);
  if (stages & 8)
    SCHRO_LAUNCH (ma_chain_kernel, dim3 (1, npics), dim3 (64), 0, stream, d_pics, scratch, 1);
  if (stages & 16)
    SCHRO_LAUNCH (ma_mode_kernel, dim3 (npics), dim3 (kMdWalkThreads), 0, stream, d_pics, scratch);
  if (stages & 32)
    SCHRO_LAUNCH (ma_chain_kernel, dim3 (kMdSections - 2, npics), dim3 (64), 0, stream, d_pics, scratch, 2);
  if (stages & 64)
    SCHRO_LAUNCH (ma_value_kernel, dim3 (npics), dim3 (kMdWalkThreads), 0, stream, d_pics, scratch);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "motion arith decode launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
