// motion_dec.hip -- the motion data of a noarith (VLC) picture, read on the device: the twin of
// schro_decoder_parse_block_data and schro_decoder_decode_block_data / _decode_macroblock / _decode_prediction_unit
// (schrodecoder.c:2531-2814) for params->is_noarith, over the predictors of schromotion.c:163-430.
//
// The reference decodes superblock by superblock and reads nine bit streams in lockstep.  Two facts break that up.
// Every neighbour a prediction reads is final: a unit at (x, y) predicts from (x - 1, y), (x, y - 1) and (x - 1, y - 1),
// each in an earlier superblock or behind a copy _decode_macroblock has made before the next unit is decoded; so the field
// is the unique solution of "unit = f (final neighbours) + residual" and any order that respects x + y computes it.  And
// residual positions depend only on earlier stages: superblock k's split residual is the k-th uint of section 0; without
// global motion unit n's mode bits lie at n * (1 + (num_refs > 1)), n a prefix sum of 1, 4 or 16 per superblock; a unit's
// code index in a vector or DC section is a prefix count, in stream order, of the units whose final mode selects it.
//
//   md_header_kernel   thread 0 of a wave per picture walks the 7 or 9 headers (byte_sync, uint, byte_sync), cuts payloads
//                      at the input's end, hands sections 0 and 2 .. 8 their chunks and writes every word of the result.
//   md_summary_kernel  a lane per 64-bit chunk: per entry state the exit state and the codes completed (na_chunks.h;
//                      section 0 carries uint codes: its machine has no sign state).
//   md_scan_kernel     a workgroup per section composes the summaries, a run of chunks per thread: per chunk the entry
//                      state and the index of the first code that starts there; per section the codes that complete and
//                      the state behind the last chunk.
//   md_extract_kernel  a lane per chunk decodes the codes that start in it, following the last one across the boundary,
//                      and stores them as 32-bit residuals at res[section][index] while index is below the section's
//                      ceiling (blocks; superblocks for section 0).  A code behind the payload is made of guard bits and
//                      is 0: the walks take 0 for an index at or behind the codes that start in the payload, so the arrays
//                      are not cleared first.
//   md_split_kernel    a workgroup per picture: splits over anti-diagonals of superblocks, then the prefix sum of 1, 4 or 16.
//   md_mode_kernel     a workgroup per picture: modes over anti-diagonals of blocks, a lane per block; unit origins
//                      compute, every block of the unit is written.  With global motion a unit's third bit exists only
//                      when its mode is not 0: thread 0 walks the units in stream order instead (correct and slow).  Then
//                      the prefix counts, in stream order, of the units that select ref-1, ref-2 and the DCs.
//   md_value_kernel    a workgroup per picture: vectors and DCs over anti-diagonals of blocks, residuals by index, whole
//                      20-byte records for every block of the unit; then the bits each section was read for and the masks.
//
// The walks are latency chains of one barrier per diagonal.  No store leaves `motion`, `result` and the scratch; input
// bytes are fetched as the aligned words that hold them (na_chunks.h).

#include "motion_common.h"
#include "na_chunks.h"
#include "motion_walks.h"

namespace schro {
namespace {

enum { kMdFirst = 0, kMdBytes, kMdChunks, kMdBase, kMdDone, kMdEnd, kMdUnits, kMdSpare };

struct MdScratch {
  uint32_t *sec, *sum, *rec, *res0, *split, *unit_first, *res, *st, *idx;
  uint32_t nsb, blocks;
};

__device__ __forceinline__ MdScratch
md_scratch (const MdPicture & pic, uint32_t * scratch)
{
  MdScratch S;
  S.blocks = (uint32_t) pic.nbx * (uint32_t) pic.nby;
  S.nsb = S.blocks >> 4;
  S.sec = scratch + pic.scratch_first;
  S.sum = S.sec + kMdSections * kMdSecWords;
  S.rec = S.sum + 2 * (size_t) pic.chunk_cap;
  S.res0 = S.rec + 2 * (size_t) pic.chunk_cap;
  S.split = S.res0 + S.nsb;
  S.unit_first = S.split + S.nsb;
  S.res = S.res0 + ((3 * (size_t) S.nsb + 1) & ~(size_t) 1);
  S.st = S.res + 7 * (size_t) S.blocks;
  S.idx = S.st + S.blocks;
  return S;
}

// the launches over chunks: grid y is one of sections 0, 2 .. 8
__device__ __forceinline__ int
md_grid_section (int j)
{
  return j ? j + 1 : 0;
}

__device__ __forceinline__ NdBits
md_section_bits (const MdPicture & pic, const uint32_t * sec)
{
  return nd_bits (pic.data, gload < uint32_t > (sec + kMdFirst), gload < uint32_t > (sec + kMdBytes));
}

// nd_walk for uint codes: the follow 1 ends the code
__device__ __forceinline__ NdWalk
md_walk_uint (uint64_t w, uint32_t off, uint32_t state, uint32_t limit)
{
  NdWalk r;
  uint32_t count = 0;
#pragma unroll 1
  while (count < limit && off < 64u) {
    if (state == kD) {
      off += 1;
      state = kF;
    } else if (state == kS) {   // (not a state of this machine: left as nd_walk leaves it)
      off += 1;
      state = kA;
      count += 1;
    } else if (state == kA) {
      const uint64_t x = ~(w << off);
      const uint32_t ones = x ? (uint32_t) __clzll ((long long) x) : 64u;
      const uint32_t z = min (min (ones, 64u - off), limit - count);
      count += z;
      off += z;
      if (z < ones || count >= limit || off >= 64u)
        continue;
      state = kF;
    } else {
      const uint64_t x = (w << off) & kFollow;
      if (x == 0) {
        state = ((64u - off) & 1u) ? kD : kF;
        off = 64u;
      } else {
        off += (uint32_t) __clzll ((long long) x) + 1u;
        state = kA;
        count += 1;
      }
    }
  }
  r.off = off;
  r.state = state;
  r.count = count;
  return r;
}

__device__ __forceinline__ NdWalk
md_walk (bool is_signed, uint64_t w, uint32_t off, uint32_t state, uint32_t limit)
{
  return is_signed ? nd_walk (w, off, state, limit) : md_walk_uint (w, off, state, limit);
}

// maps of the four states with 64-bit counts (a section of 2^32 bits can hold 2^32 codes)
__device__ __forceinline__ uint64_t
md_pick (const uint64_t f[4], uint32_t s)
{
  return s == 0 ? f[0] : s == 1 ? f[1] : s == 2 ? f[2] : f[3];
}

__device__ __forceinline__ void
md_compose (uint64_t out[4], const uint64_t first[4], const uint64_t then[4])
{
#pragma unroll
  for (int s = 0; s < 4; s++)
    out[s] = (first[s] & ~3ull) + md_pick (then, (uint32_t) first[s] & 3u);
}

__device__ __forceinline__ void
md_load_sum (uint64_t t[4], const uint32_t * sum, size_t slot)
{
  const u32x2 v = gload < u32x2 > (sum + 2 * slot);
  t[0] = v.x & 0xffffu;
  t[1] = v.x >> 16;
  t[2] = v.y & 0xffffu;
  t[3] = v.y >> 16;
}

__device__ __forceinline__ uint32_t
md_sat32 (uint64_t v)
{
  return v > 0xffffffffull ? 0xffffffffu : (uint32_t) v;
}

// the codes of a section that start in its payload's chunks: those that complete there and the one under way at the end
__device__ __forceinline__ uint32_t
md_started (const uint32_t * sec)
{
  return md_sat32 ((uint64_t) gload < uint32_t > (sec + kMdDone) + (gload < uint32_t > (sec + kMdEnd) != kA ? 1u : 0u));
}

// ---- header ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (64)
void md_header_kernel (const MdPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  if (threadIdx.x != 0)
    return;
  const MdPicture & pic = pics[blockIdx.x];
  const MdScratch S = md_scratch (pic, scratch);
  SchroHipMotionDecodeResult *res = pic.result;
  uint32_t L = pic.data_bytes;
  if (pic.bytes_on_device)
    L = min (L, gload < uint32_t > (pic.bytes_on_device));
  const NdBits O = nd_bits (pic.data, 0, L);
  uint64_t pos = 0;
  uint32_t longs = 0, truncated = 0, chunk = 0;
#pragma unroll 1
  for (int s = 0; s < kMdSections; s++) {
    uint32_t first = 0, bytes = 0, nchunks = 0;
    if (!(pic.num_refs < 2 && (s == 4 || s == 5))) {
      pos = (pos + 7u) & ~7ull;
      const uint32_t length = nd_code (O, pos, longs, false);
      pos = (pos + 7u) & ~7ull;
      const uint64_t fb = pos >> 3;
      bytes = fb < L ? min (length, L - (uint32_t) fb) : 0u;
      truncated |= (bytes < length ? 1u : 0u) << s;
      pos += 8ull * length;
      first = bytes ? (uint32_t) fb : 0u;
      nchunks = s == 1 ? 0u : (bytes + 7u) >> 3;
    }
    uint32_t *sec = S.sec + s * kMdSecWords;
    gstore < uint32_t > (sec + kMdFirst, first);
    gstore < uint32_t > (sec + kMdBytes, bytes);
    gstore < uint32_t > (sec + kMdChunks, nchunks);
    gstore < uint32_t > (sec + kMdBase, chunk);
    gstore < uint32_t > (sec + kMdDone, 0u);
    gstore < uint32_t > (sec + kMdEnd, (uint32_t) kA);
    gstore < uint32_t > (sec + kMdUnits, 0u);
    gstore < uint32_t > (sec + kMdSpare, 0u);
    chunk += nchunks;
    gstore < uint32_t > (&res->section_bytes[s], bytes);
    gstore < uint32_t > (&res->section_units[s], 0u);
    gstore < uint32_t > (&res->section_bits[s], 0u);
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

// ---- summary -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (kMdLaneThreads)
void md_summary_kernel (const MdPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  const MdPicture & pic = pics[blockIdx.z];
  const MdScratch S = md_scratch (pic, scratch);
  const int s = md_grid_section ((int) blockIdx.y);
  const uint32_t *sec = S.sec + s * kMdSecWords;
  const uint32_t q = (uint32_t) blockIdx.x * kMdLaneThreads + threadIdx.x;
  if (q >= gload < uint32_t > (sec + kMdChunks))
    return;
  const uint64_t w = nd_bits64 (md_section_bits (pic, sec), 64ull * q);
  uint32_t e[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const NdWalk r = md_walk (s != 0, w, 0, k, 0xffffffffu);
    e[k] = (r.count << 2) | r.state;
  }
  u32x2 sum;
  sum.x = e[0] | (e[1] << 16);
  sum.y = e[2] | (e[3] << 16);
  gstore < u32x2 > (S.sum + 2 * ((size_t) gload < uint32_t > (sec + kMdBase) + q), sum);
}

// ---- scan --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (kMdScanThreads)
void md_scan_kernel (const MdPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  __shared__ uint64_t part[4][kMdScanThreads];
  const MdPicture & pic = pics[blockIdx.y];
  const MdScratch S = md_scratch (pic, scratch);
  const int s = md_grid_section ((int) blockIdx.x);
  uint32_t *sec = S.sec + s * kMdSecWords;
  const uint32_t nchunks = gload < uint32_t > (sec + kMdChunks);
  const size_t slot0 = gload < uint32_t > (sec + kMdBase);
  const int tid = (int) threadIdx.x, T = kMdScanThreads;
  // a run of chunks per thread
  const uint32_t run = (nchunks + (uint32_t) T - 1u) / (uint32_t) T;
  const uint32_t c0 = min (nchunks, (uint32_t) tid * run), c1 = min (nchunks, c0 + run);
  uint64_t f[4] = { kA, kD, kF, kS };   // the identity
#pragma unroll 1
  for (uint32_t c = c0; c < c1; c++) {
    uint64_t t[4], o[4];
    md_load_sum (t, S.sum, slot0 + c);
    md_compose (o, f, t);
#pragma unroll
    for (int k = 0; k < 4; k++)
      f[k] = o[k];
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
    part[k][tid] = f[k];
  __syncthreads ();
  // the inclusive scan of the runs' maps
  for (int d = 1; d < T; d <<= 1) {
    uint64_t o[4] = { kA, kD, kF, kS }, t[4];
    if (tid >= d) {
#pragma unroll
      for (int k = 0; k < 4; k++)
        o[k] = part[k][tid - d];
    }
    __syncthreads ();
    md_compose (t, o, f);
#pragma unroll
    for (int k = 0; k < 4; k++)
      part[k][tid] = f[k] = t[k];
    __syncthreads ();
  }
  // a section is entered at a code's start
  const uint64_t in = tid ? part[kA][tid - 1] : (uint64_t) kA;
  uint64_t done = in >> 2;
  uint32_t state = (uint32_t) in & 3u;
#pragma unroll 1
  for (uint32_t c = c0; c < c1; c++) {
    gstore < uint32_t > (S.rec + 2 * (slot0 + c), md_sat32 (done + (state != kA ? 1u : 0u)));
    gstore < uint32_t > (S.rec + 2 * (slot0 + c) + 1, state);
    uint64_t t[4];
    md_load_sum (t, S.sum, slot0 + c);
    const uint64_t e = md_pick (t, state);
    done += e >> 2;
    state = (uint32_t) e & 3u;
  }
  if (tid == T - 1) {
    gstore < uint32_t > (sec + kMdDone, md_sat32 (f[kA] >> 2));
    gstore < uint32_t > (sec + kMdEnd, (uint32_t) f[kA] & 3u);
  }
}

// ---- extract -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (kMdLaneThreads)
void md_extract_kernel (const MdPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  const MdPicture & pic = pics[blockIdx.z];
  const MdScratch S = md_scratch (pic, scratch);
  const int s = md_grid_section ((int) blockIdx.y);
  const uint32_t *sec = S.sec + s * kMdSecWords;
  const uint32_t q = (uint32_t) blockIdx.x * kMdLaneThreads + threadIdx.x;
  if (q >= gload < uint32_t > (sec + kMdChunks))
    return;
  const size_t slot = (size_t) gload < uint32_t > (sec + kMdBase) + q;
  uint32_t n = gload < uint32_t > (S.rec + 2 * slot);
  const uint32_t entry = gload < uint32_t > (S.rec + 2 * slot + 1);
  const uint32_t ceiling = s ? S.blocks : S.nsb;
  if (n >= ceiling)
    return;
  const NdBits B = md_section_bits (pic, sec);
  const uint64_t begin = 64ull * q, end = begin + 64u;
  uint64_t pos = begin;
  if (entry != kA) {
    // the rest of a code that started before
    const NdWalk r = md_walk (s != 0, nd_bits64 (B, begin), 0, entry, 1u);
    if (r.count == 0)
      return;
    pos = begin + r.off;
  }
  uint32_t *out = s ? S.res + (size_t) (s - 2) * S.blocks : S.res0;
  uint32_t longs = 0;
#pragma unroll 1
  while (pos < end && n < ceiling) {
    const uint32_t m = nd_code (B, pos, longs, s != 0);
    gstore < uint32_t > (out + n, m);
    n++;
  }
  if (longs)
    atomicAdd (&pic.result->long_codes, longs);
}

// ---- the walks -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (kMdSplitThreads)
void md_split_kernel (const MdPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  __shared__ uint32_t part[kMdSplitThreads];
  const MdPicture & pic = pics[blockIdx.x];
  const MdScratch S = md_scratch (pic, scratch);
  const int nsbx = pic.nbx >> 2, nsby = pic.nby >> 2, nsb = (int) S.nsb;
  const int tid = (int) threadIdx.x, T = kMdSplitThreads;
  const uint32_t have = min (md_started (S.sec), S.nsb);
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
      const uint32_t value = (uint32_t) k < have ? gload < uint32_t > (S.res0 + k) : 0u;
      gstore < uint32_t > (S.split + k, (uint32_t) (((uint64_t) pred + value) % 3u));
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
    gstore < uint32_t > (S.sec + 0 * kMdSecWords + kMdUnits, S.nsb);
    gstore < uint32_t > (S.sec + 1 * kMdSecWords + kMdUnits, part[tid]);
    gstore < uint32_t > (&pic.result->section_units[0], S.nsb);
    gstore < uint32_t > (&pic.result->section_units[1], part[tid]);
  }
}

__global__ __launch_bounds__ (kMdWalkThreads)
void md_mode_kernel (const MdPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  __shared__ uint32_t part[3 * kMdWalkThreads];
  const MdPicture & pic = pics[blockIdx.x];
  const MdScratch S = md_scratch (pic, scratch);
  const int nbx = pic.nbx, nsbx = nbx >> 2, nsb = (int) S.nsb;
  const int tid = (int) threadIdx.x, T = kMdWalkThreads;
  const NdBits B = md_section_bits (pic, S.sec + 1 * kMdSecWords);
  const uint32_t bits = pic.num_refs > 1 ? 2u : 1u;
  if (!pic.have_global) {
    walk_diagonals (nbx, pic.nby, tid, T, [&](int x, int y) {
        const int sb = (y >> 2) * nsbx + (x >> 2);
        const uint32_t split = gload < uint32_t > (S.split + sb);
        const int step = 4 >> split;
        if ((x | y) & (step - 1))
          return;               // not a unit's origin
        const uint32_t n = gload < uint32_t > (S.unit_first + sb) + ((((uint32_t) y & 3u) >> (2u - split)) << split) + (((uint32_t) x & 3u) >> (2u - split));
        const uint64_t w = nd_bits64 (B, (uint64_t) n * bits);
        uint32_t r = (uint32_t) (w >> 63);
        if (bits > 1)
          r |= (uint32_t) (w >> 62 & 1u) << 1;
        const uint32_t mode = (md_majority (S.st, nbx, x, y) ^ r) & 3u;
        md_store_unit (S.st, nbx, x, y, step, mode | (split << 3));
    });
    if (tid == 0) {
      const uint64_t read = (uint64_t) gload < uint32_t > (S.sec + 1 * kMdSecWords + kMdUnits) * bits;
      gstore < uint32_t > (&pic.result->section_bits[1], md_sat32 (read));
    }
  } else {
    if (tid == 0) {
      uint64_t pos = 0;
#pragma unroll 1
      for (int sb = 0; sb < nsb; sb++) {
        const uint32_t split = gload < uint32_t > (S.split + sb);
        md_units (nsbx, sb, split, [&](int x, int y) {
            const uint32_t maj = md_majority (S.st, nbx, x, y);
            const uint64_t w = nd_bits64 (B, pos);
            uint32_t r = (uint32_t) (w >> 63);
            if (bits > 1)
              r |= (uint32_t) (w >> 62 & 1u) << 1;
            pos += bits;
            const uint32_t mode = (maj ^ r) & 3u;
            uint32_t ug = 0;
            if (mode) {
              ug = ((maj >> 2) ^ (uint32_t) (w >> (63u - bits))) & 1u;
              pos += 1;
            }
            md_store_unit (S.st, nbx, x, y, 4 >> split, mode | (ug << 2) | (split << 3));
        });
      }
      gstore < uint32_t > (&pic.result->section_bits[1], md_sat32 (pos));
    }
    __syncthreads ();
  }

  // which code of its sections a unit owns: the counts, in stream order, of the units before it that select ref-1, ref-2
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
      const uint32_t units = part[(s < 4 ? 0 : s < 6 ? 1 : 2) * T + tid];
      gstore < uint32_t > (S.sec + s * kMdSecWords + kMdUnits, units);
      gstore < uint32_t > (&pic.result->section_units[s], units);
    }
  }
}

// the bits a VLC section was read for when the field asked it for `units` codes
__device__ __forceinline__ uint64_t
md_bits_read (const MdPicture & pic, const MdScratch & S, int s, uint32_t units)
{
  const uint32_t *sec = S.sec + s * kMdSecWords;
  const bool is_signed = s != 0;
  if (units == 0)
    return 0;
  const uint32_t nchunks = gload < uint32_t > (sec + kMdChunks), end = gload < uint32_t > (sec + kMdEnd);
  const uint32_t started = md_started (sec);
  if (units > started) {
    // behind the payload every bit reads 1: the code under way ends on guard bits, every further one takes a bit
    const uint32_t tail = end == kD ? (is_signed ? 3u : 2u) : end == kF ? (is_signed ? 2u : 1u) : end == kS ? 1u : 0u;
    return 64ull * nchunks + tail + (units - started);
  }
  // the last chunk whose first code is at or before the last one asked for: that code starts there
  const uint32_t *rec = S.rec + 2 * (size_t) gload < uint32_t > (sec + kMdBase);
  uint32_t lo = 0, hi = nchunks - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (gload < uint32_t > (rec + 2 * (size_t) mid) <= units - 1)
      lo = mid;
    else
      hi = mid - 1;
  }
  const NdBits B = md_section_bits (pic, sec);
  uint64_t pos = 64ull * lo;
  const uint32_t entry = gload < uint32_t > (rec + 2 * (size_t) lo + 1);
  if (entry != kA)
    pos += md_walk (is_signed, nd_bits64 (B, pos), 0, entry, 1u).off;
  uint32_t none = 0;
  for (uint32_t n = gload < uint32_t > (rec + 2 * (size_t) lo); n < units; n++)
    (void) nd_code (B, pos, none, is_signed);
  return pos;
}

__global__ __launch_bounds__ (kMdWalkThreads)
void md_value_kernel (const MdPicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  __shared__ uint32_t tot_unverified, tot_first, overran, not_consumed;
  const MdPicture & pic = pics[blockIdx.x];
  const MdScratch S = md_scratch (pic, scratch);
  const int nbx = pic.nbx;
  const int tid = (int) threadIdx.x, T = kMdWalkThreads;
  uint8_t *field = pic.motion;
  if (tid == 0)
    tot_unverified = 0, tot_first = 0xffffffffu, overran = 0, not_consumed = 0;
  uint32_t have[7];
#pragma unroll
  for (int k = 0; k < 7; k++)
    have[k] = min (md_started (S.sec + (2 + k) * kMdSecWords), S.blocks);
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
          const uint32_t r = ia < have[4 + i] ? gload < uint32_t > (S.res + (size_t) (4 + i) * S.blocks + ia) : 0u;
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
            const uint32_t rx = i < have[2 * ref] ? gload < uint32_t > (S.res + (size_t) (2 * ref) * S.blocks + i) : 0u;
            const uint32_t ry = i < have[2 * ref + 1] ? gload < uint32_t > (S.res + (size_t) (2 * ref + 1) * S.blocks + i) : 0u;
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
  // what each section was read for (the modes' bits: md_mode_kernel)
  if (tid < kMdSections) {
    const int s = tid;
    const uint32_t *sec = S.sec + s * kMdSecWords;
    const bool absent = pic.num_refs < 2 && (s == 4 || s == 5);
    uint64_t read = 0;
    if (s == 1)
      read = gload < uint32_t > (&pic.result->section_bits[1]);
    else if (!absent)
      read = md_bits_read (pic, S, s, gload < uint32_t > (sec + kMdUnits));
    const uint64_t kept = 8ull * gload < uint32_t > (sec + kMdBytes);
    if (s != 1)
      gstore < uint32_t > (&pic.result->section_bits[s], md_sat32 (read));
    if (read > kept)
      atomicOr (&overran, 1u << s);
    if (read + 8u <= kept)
      atomicOr (&not_consumed, 1u << s);
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
launch_motion_decode (hipStream_t stream, const MdPicture * d_pics, int npics, uint32_t * scratch, int lane_x, int stages)
{
  if (stages & 1)
    SCHRO_LAUNCH (md_header_kernel, dim3 (npics), dim3 (64), 0, stream, d_pics, scratch);
  if (stages & 2)
    SCHRO_LAUNCH (md_summary_kernel, dim3 (lane_x, kMdSections - 1, npics), dim3 (kMdLaneThreads), 0, stream, d_pics, scratch);
  if (stages & 4)
    SCHRO_LAUNCH (md_scan_kernel, dim3 (kMdSections - 1, npics), dim3 (kMdScanThreads), 0, stream, d_pics, scratch);
  if (stages & 8)
    SCHRO_LAUNCH (md_extract_kernel, dim3 (lane_x, kMdSections - 1, npics), dim3 (kMdLaneThreads), 0, stream, d_pics, scratch);
  if (stages & 16)
    SCHRO_LAUNCH (md_split_kernel, dim3 (npics), dim3 (kMdSplitThreads), 0, stream, d_pics, scratch);
  if (stages & 32)
    SCHRO_LAUNCH (md_mode_kernel, dim3 (npics), dim3 (kMdWalkThreads), 0, stream, d_pics, scratch);
  if (stages & 64)
    SCHRO_LAUNCH (md_value_kernel, dim3 (npics), dim3 (kMdWalkThreads), 0, stream, d_pics, scratch);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "motion decode launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
