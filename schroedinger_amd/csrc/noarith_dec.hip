// noarith_dec.hip -- core-syntax transform data in the VLC parse codes, read on the device: the twin of
// schro_decoder_parse_transform_data (schrodecoder.c:2939-2987) and schro_decoder_decode_transform_data (:2990-3015) over
// schro_decoder_decode_subband (:3525-3625) and schro_decoder_decode_codeblock_noarith (:3355-3449).  These are the
// DECODER's rules for zero flags and quant offsets; the encoder's (noarith_enc.hip) differ, see schro_hip.h.
//
// The code has no contexts: the only thing carried from value to value is the bit position.  It is a four-state machine
// over bits, MSB first -- A code start (1: the code is done, value 0; 0: D), D data bit (any: F), F follow bit (0: D, 1: S),
// S sign bit (any: A, the code is done).  The unit is the CHUNK: 64 bits of a sub-band's payload, counted from its first
// byte.  A chunk's summary is, per entry state, the exit state and the codes completed in it; summaries compose
// associatively, so where every codeblock starts follows from scans, and every chunk can then be decoded on its own.
//
//   nd_header_kernel   thread 0 of a wave per picture walks the serial chain of at most 57 sub-band headers, runs the
//                      compat test (a peeked sint per component), cuts payloads at the input's end, hands every coded
//                      sub-band its chunks and writes the header part of the result.
//   nd_summary_kernel  a lane per chunk: the summary (8 bytes) by runs (__clzll), not bit by bit; marks the chunk's record
//                      as empty.
//   nd_chain_kernel    a workgroup per coded sub-band.  Its codeblocks are a serial chain -- each one's first bit is the
//                      previous one's end.  Thread 0 reads a codeblock's head (flag, offset) and walks to the chunk's end;
//                      if the codeblock's width x height codes are not complete by then the workgroup composes the stored
//                      summaries of the following chunks, kNdChainThreads per step (__shfl_up within a wave, LDS across
//                      waves), until the count is reached, and thread 0 finishes inside that chunk.  It writes a record
//                      per codeblock (first value bit -- the flag's bit when zero --, quant index, zero) and per chunk (the codeblock, the index of the
//                      first code that starts there, the entry state).
//   nd_decode_kernel   a lane per chunk decodes the codes that START in its chunk, following the last one across the
//                      boundary (to the payload's end at most: behind it every bit reads 1), moves on to the next
//                      codeblock while that one's first value bit lies in the chunk, dequantises (dequant_one.h) and stores.
//   nd_fill_kernel     a wave per row piece of a codeblock: zero sub-bands, zero codeblocks, and the values behind the
//                      payload's end.
//
// Outside nd_header_kernel and thread 0's head step no trip count grows with the stream: a lane sees at most 64 codes and
// 64 heads per chunk and one code's tail.  Nothing is read outside the aligned dwords that hold the input's bytes, and
// nothing of a picture whose header walk set the error is written.

#include "schro_hip_internal.h"
#include "dequant_one.h"
#include "na_chunks.h"

namespace schro {
namespace {

// the picture's chunk q belongs to sub-band ...: the last one whose chunk_base is <= q (a sub-band without chunks shares
// its base with the next one)
__device__ __forceinline__ int
nd_find (const uint32_t * base, int nsb, uint32_t q)
{
  int lo = 0, hi = nsb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base[mid] <= q)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

struct NdGeo {
  int xmin, ymin, w, h;
};

__device__ __forceinline__ NdGeo
nd_geo (const NdSubband & sb, uint32_t c)
{
  NdGeo g;
  const int y = (int) (c / (uint32_t) sb.hc), x = (int) (c - (uint32_t) y * (uint32_t) sb.hc);
  g.xmin = (x * sb.bw) / sb.hc;
  g.ymin = (y * sb.bh) / sb.vc;
  g.w = ((x + 1) * sb.bw) / sb.hc - g.xmin;
  g.h = ((y + 1) * sb.bh) / sb.vc - g.ymin;
  return g;
}

// ---- header ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (64)
void nd_header_kernel (const NdSubband * __restrict__ sbs, const NdPicture * __restrict__ pics, const NdScratch S)
{
  if (threadIdx.x != 0)
    return;
  const NdPicture & pic = pics[blockIdx.x];
  SchroHipNoarithDecodeResult *res = pic.result;
  uint32_t L = pic.data_bytes;
  if (pic.bytes_on_device)
    L = min (L, gload < uint32_t > (pic.bytes_on_device));
  const NdBits O = nd_bits (pic.data, 0, L);
  uint64_t pos = 0;
  uint32_t longs = 0, truncated = 0, chunk = 0, error = 0, compat = pic.compat ? 1u : 0u;
#pragma unroll 1
  for (int s = 0; s < pic.nsb; s++) {
    const NdSubband & sb = sbs[pic.sb_first + s];
    NdBand band;
    band.first_byte = band.bytes = band.length = band.nchunks = band.quant_index = band.flags = band.pad = 0;
    band.chunk_base = chunk;
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
          // schro_decoder_test_quant_offset_compat: a codeblock of a 1 x 1 sub-band has no zero flag in front of the offset
          if (qo && one && sb.index == 0) {
            const NdBits P = nd_bits (pic.data, avail ? (uint32_t) fb : 0u, avail);
            uint64_t at = 0;
            uint32_t none = 0;
            const int64_t q = (int64_t) qi + (int32_t) nd_code (P, at, none, true);
            if (q < 0 || q > 60) {
              compat = 1;
              qo = false;
            }
          }
          band.first_byte = avail ? (uint32_t) fb : 0u;
          band.bytes = avail;
          band.length = length;
          band.nchunks = (avail + 7u) >> 3;
          band.quant_index = qi;
          band.flags = 1u | (one ? 0u : 2u) | (qo ? 4u : 0u);
          chunk += band.nchunks;
          gstore < uint32_t > (&res->subband_length[sb.comp][sb.index], length);
          gstore < uint8_t > (&res->subband_quant_index[sb.comp][sb.index], (uint8_t) qi);
        }
      }
    }
    uint32_t *out = (uint32_t *) (S.bands + pic.sb_first + s);
    const uint32_t *in = (const uint32_t *) &band;
#pragma unroll
    for (int k = 0; k < kNdBandWords; k++)
      gstore < uint32_t > (out + k, in[k]);
  }
  if (!error)
    pos = (pos + 7u) & ~7ull;
  const uint64_t bytes_read = (pos + 7u) >> 3;
  gstore < uint32_t > (&res->bytes_read, bytes_read > 0xffffffffull ? 0xffffffffu : (uint32_t) bytes_read);
  gstore < uint32_t > (&res->compat_quant_offset, error ? (pic.compat ? 1u : 0u) : compat);
  gstore < uint32_t > (&res->truncated, truncated);
  gstore < uint32_t > (&res->long_codes, longs);
  gstore < uint32_t > (S.ptotal + kNdPicWords * blockIdx.x, error ? 0u : chunk);
}

// ---- summary -----------------------------------------------------------------------------------------------------------

// the picture's sub-band tables to LDS; true when chunk q of the picture exists
__device__ __forceinline__ void
nd_load_bases (uint32_t * base, const NdPicture & pic, const NdScratch & S)
{
  for (int k = (int) threadIdx.x; k < pic.nsb; k += (int) blockDim.x)
    base[k] = gload < uint32_t > (&S.bands[pic.sb_first + k].chunk_base);
  __syncthreads ();
}

__global__ __launch_bounds__ (kNdLaneThreads)
void nd_summary_kernel (const NdPicture * __restrict__ pics, const NdScratch S)
{
  __shared__ uint32_t base[kNaMaxSubbands];
  const NdPicture & pic = pics[blockIdx.y];
  const uint32_t total = gload < uint32_t > (S.ptotal + kNdPicWords * blockIdx.y);
  if ((uint32_t) blockIdx.x * kNdLaneThreads >= total)
    return;
  nd_load_bases (base, pic, S);
  const uint32_t q = (uint32_t) blockIdx.x * kNdLaneThreads + threadIdx.x;
  if (q >= total)
    return;
  const NdBand & band = S.bands[pic.sb_first + nd_find (base, pic.nsb, q)];
  const NdBits B = nd_bits (pic.data, gload < uint32_t > (&band.first_byte), gload < uint32_t > (&band.bytes));
  const uint64_t w = nd_bits64 (B, 64ull * (q - gload < uint32_t > (&band.chunk_base)));
  uint32_t e[4];
#pragma unroll
  for (uint32_t s = 0; s < 4; s++) {
    const NdWalk r = nd_walk (w, 0, s, 0xffffffffu);
    e[s] = (r.count << 2) | r.state;
  }
  const size_t slot = (size_t) pic.chunk_first + q;
  u32x2 sum;
  sum.x = e[0] | (e[1] << 16);
  sum.y = e[2] | (e[3] << 16);
  gstore < u32x2 > (S.sum + 2 * slot, sum);
  gstore < uint32_t > (S.rec + 3 * slot, kNaNone);
}

// ---- chain -------------------------------------------------------------------------------------------------------------

struct NdChain {
  uint64_t pos;                 // the next bit of the payload
  uint32_t c;                   // the next codeblock
  int32_t qi;                   // the carried quant index
  int32_t rec_hi;               // the last chunk that has its record
  uint32_t scan;                // 1: the workgroup scans on for codeblock c
  uint32_t scan_chunk, entry, done, need;       // from this chunk, entered in this state, with this many of `need` codes complete
  uint32_t found, fin_chunk, fin_entry, fin_before;
  uint32_t last_state, last_count;      // behind the payload's last chunk
  uint32_t end_state, end_count;        // behind the step's last chunk
};

__global__ __launch_bounds__ (kNdChainThreads)
void nd_chain_kernel (const NdSubband * __restrict__ sbs, const NdPicture * __restrict__ pics, const NdScratch S)
{
  __shared__ NdChain sh;
  __shared__ uint32_t wave_map[kNdChainThreads / 64][4];
  const NdSubband & sb = sbs[blockIdx.x];
  const NdPicture & pic = pics[sb.pic];
  if (gload < uint32_t > (&pic.result->error))
    return;
  const NdBand & bd = S.bands[blockIdx.x];
  const uint32_t flags = gload < uint32_t > (&bd.flags);
  if (!(flags & 1u))
    return;
  const uint32_t nchunks = gload < uint32_t > (&bd.nchunks), length = gload < uint32_t > (&bd.length);
  const NdBits B = nd_bits (pic.data, gload < uint32_t > (&bd.first_byte), gload < uint32_t > (&bd.bytes));
  const size_t slot0 = (size_t) pic.chunk_first + gload < uint32_t > (&bd.chunk_base);
  const uint32_t *sum = S.sum + 2 * slot0;
  uint32_t *rec = S.rec + 3 * slot0;
  uint32_t *cbr = S.cb + (size_t) kNdCbWords * (size_t) sb.cb_base;
  const uint32_t ncb = (uint32_t) sb.hc * (uint32_t) sb.vc;
  const bool zf = flags & 2u, qo = flags & 4u;
  const int tid = (int) threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t longs = 0, clamped = 0;      // thread 0's
  if (tid == 0) {
    sh.pos = 0;
    sh.c = 0;
    sh.qi = (int32_t) gload < uint32_t > (&bd.quant_index);
    sh.rec_hi = -1;
    sh.found = 0;
  }
  __syncthreads ();
#pragma unroll 1
  for (;;) {
    // the head step: codeblocks that end in the chunk they start in
    if (tid == 0) {
      uint64_t pos = sh.pos;
      uint32_t c = sh.c;
      int32_t qi = sh.qi, rec_hi = sh.rec_hi;
      uint32_t scan = 0;
#pragma unroll 1
      while (c < ncb) {
        const NdGeo g = nd_geo (sb, c);
        const uint32_t need = (uint32_t) g.w * (uint32_t) g.h;
        uint32_t *cr = cbr + (size_t) kNdCbWords * c;
        if (zf) {
          const uint32_t bit = (uint32_t) (nd_bits64 (B, pos) >> 63);
          pos += 1;
          if (bit) {
            gstore < uint32_t > (cr + 0, nd_sat32 (pos - 1));        // (the flag's bit: a decode lane stops at a head behind its chunk)
            gstore < uint32_t > (cr + 1, (uint32_t) qi | 0x100u);
            gstore < uint32_t > (cr + 2, 0u);
            c++;
            continue;
          }
        }
        if (qo) {
          const int64_t q = (int64_t) qi + (int32_t) nd_code (B, pos, longs, true);
          qi = (int32_t) (q < 0 ? 0 : q > 60 ? 60 : q);
          clamped += q != qi;
        }
        uint32_t ncoded = need;
        const uint64_t first = pos;
        bool go_on = true;
        if (need == 0) {
        } else if (pos >= 64ull * nchunks) {
          // behind the payload every bit reads 1: each value is 0 and takes a bit
          ncoded = 0;
          pos += need;
        } else {
          const uint32_t j = (uint32_t) (pos >> 6), off = (uint32_t) pos & 63u;
          if ((int32_t) j > rec_hi) {
            gstore < uint32_t > (rec + 3 * (size_t) j + 0, c);
            gstore < uint32_t > (rec + 3 * (size_t) j + 1, 0u);
            gstore < uint32_t > (rec + 3 * (size_t) j + 2, (uint32_t) kA | (off << 2));
            rec_hi = (int32_t) j;
          }
          const NdWalk r = nd_walk (nd_bits64 (B, 64ull * j), off, kA, need);
          if (r.count == need) {
            pos = 64ull * j + r.off;
          } else if (j + 1 >= nchunks) {
            // the payload ends inside the codeblock: the code under way ends on guard bits, the rest are 0
            ncoded = r.count + (r.state != kA);
            pos = 64ull * nchunks + (r.state == kD ? 3u : r.state == kF ? 2u : r.state == kS ? 1u : 0u) + (need - ncoded);
          } else {
            sh.scan_chunk = j + 1;
            sh.entry = r.state;
            sh.done = r.count;
            sh.need = need;
            scan = 1;
            go_on = false;
          }
        }
        gstore < uint32_t > (cr + 0, nd_sat32 (first));
        gstore < uint32_t > (cr + 1, (uint32_t) qi);
        gstore < uint32_t > (cr + 2, ncoded);
        if (!go_on)
          break;
        c++;
      }
      sh.pos = pos;
      sh.c = c;
      sh.qi = qi;
      sh.rec_hi = rec_hi;
      sh.scan = scan;
      sh.found = 0;
    }
    __syncthreads ();
    if (!sh.scan)
      break;
    // the scan: kNdChainThreads chunks per step until codeblock c's count is reached
#pragma unroll 1
    for (;;) {
      const uint32_t base = sh.scan_chunk, entry = sh.entry, done = sh.done, need = sh.need, c = sh.c;
      const uint32_t m = base + (uint32_t) tid;
      uint32_t f[4] = { kA, kD, kF, kS };       // the identity
      if (m < nchunks) {
        const u32x2 v = gload < u32x2 > (sum + 2 * (size_t) m);
        f[0] = v.x & 0xffffu;
        f[1] = v.x >> 16;
        f[2] = v.y & 0xffffu;
        f[3] = v.y >> 16;
      }
      // inclusive within the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        uint32_t o[4], t[4];
#pragma unroll
        for (int s = 0; s < 4; s++)
          o[s] = (uint32_t) __shfl_up ((int) f[s], d);
        nd_compose (t, o, f);
        if (lane >= d) {
#pragma unroll
          for (int s = 0; s < 4; s++)
            f[s] = t[s];
        }
      }
      uint32_t ex[4];           // the wave's chunks before this one
#pragma unroll
      for (int s = 0; s < 4; s++) {
        ex[s] = (uint32_t) __shfl_up ((int) f[s], 1);
        if (lane == 0)
          ex[s] = (uint32_t) s;
      }
      if (lane == 63) {
#pragma unroll
        for (int s = 0; s < 4; s++)
          wave_map[wave][s] = f[s];
      }
      __syncthreads ();
      uint32_t p[4] = { kA, kD, kF, kS };       // the waves before this one
#pragma unroll 1
      for (int k = 0; k < wave; k++) {
        uint32_t t[4], w4[4];
#pragma unroll
        for (int s = 0; s < 4; s++)
          w4[s] = wave_map[k][s];
        nd_compose (t, p, w4);
#pragma unroll
        for (int s = 0; s < 4; s++)
          p[s] = t[s];
      }
      uint32_t in[4], out[4];
      nd_compose (in, p, ex);
      nd_compose (out, p, f);
      const uint32_t ein = nd_pick (in, entry), eout = nd_pick (out, entry);
      const uint32_t es = ein & 3u, before = done + (ein >> 2), after = done + (eout >> 2);
      const bool live = m < nchunks && before < need;
      if (live) {
        gstore < uint32_t > (rec + 3 * (size_t) m + 0, c);
        gstore < uint32_t > (rec + 3 * (size_t) m + 1, before + (es != kA));
        gstore < uint32_t > (rec + 3 * (size_t) m + 2, es);
        if (after >= need) {
          sh.found = 1;
          sh.fin_chunk = m;
          sh.fin_entry = es;
          sh.fin_before = before;
        }
      }
      if (m + 1 == nchunks) {
        sh.last_state = eout & 3u;
        sh.last_count = after;
      }
      if (tid == kNdChainThreads - 1) {
        sh.end_state = eout & 3u;
        sh.end_count = after;
      }
      __syncthreads ();
      const bool found = sh.found, ended = base + kNdChainThreads >= nchunks;
      if (tid == 0) {
        if (found) {
          const NdWalk r = nd_walk (nd_bits64 (B, 64ull * sh.fin_chunk), 0, sh.fin_entry, need - sh.fin_before);
          sh.pos = 64ull * sh.fin_chunk + r.off;
          sh.rec_hi = (int32_t) sh.fin_chunk;
          sh.c = c + 1;
        } else if (ended) {
          const uint32_t e = sh.last_state, ncoded = sh.last_count + (e != kA);
          gstore < uint32_t > (cbr + (size_t) kNdCbWords * c + 2, ncoded);
          sh.pos = 64ull * nchunks + (e == kD ? 3u : e == kF ? 2u : e == kS ? 1u : 0u) + (need - ncoded);
          sh.rec_hi = (int32_t) nchunks - 1;
          sh.c = c + 1;
        } else {
          sh.scan_chunk = base + kNdChainThreads;
          sh.entry = sh.end_state;
          sh.done = sh.end_count;
        }
      }
      __syncthreads ();
      if (found || ended)
        break;
    }
  }
  if (tid == 0) {
    // what the reference warns about (:3606-3622)
    const uint64_t offset = sh.pos >> 3;
    if (offset + 1 < (uint64_t) length)
      atomicAdd (&pic.result->not_consumed, 1u);
    if (offset > (uint64_t) length)
      atomicAdd (&pic.result->overran, 1u);
    if (longs)
      atomicAdd (&pic.result->long_codes, longs);
    if (clamped)
      atomicAdd (&pic.result->clamped_quant, clamped);
  }
}

// ---- decode ------------------------------------------------------------------------------------------------------------

template < typename T, int ARITH >
__global__ __launch_bounds__ (kNdLaneThreads)
void nd_decode_kernel (const NdSubband * __restrict__ sbs, const NdPicture * __restrict__ pics, const NdScratch S)
{
  __shared__ uint32_t base[kNaMaxSubbands];
  const NdPicture & pic = pics[blockIdx.y];
  const uint32_t total = gload < uint32_t > (S.ptotal + kNdPicWords * blockIdx.y);
  if ((uint32_t) blockIdx.x * kNdLaneThreads >= total)
    return;                     // (an error picture has no chunks)
  nd_load_bases (base, pic, S);
  const uint32_t q = (uint32_t) blockIdx.x * kNdLaneThreads + threadIdx.x;
  if (q >= total)
    return;
  const int si = pic.sb_first + nd_find (base, pic.nsb, q);
  const NdSubband & sb = sbs[si];
  const NdBand & bd = S.bands[si];
  const size_t slot = (size_t) pic.chunk_first + q;
  uint32_t c = gload < uint32_t > (S.rec + 3 * slot);
  if (c == kNaNone)
    return;
  uint32_t n = gload < uint32_t > (S.rec + 3 * slot + 1);
  const uint32_t word = gload < uint32_t > (S.rec + 3 * slot + 2);
  const NdBits B = nd_bits (pic.data, gload < uint32_t > (&bd.first_byte), gload < uint32_t > (&bd.bytes));
  const uint64_t begin = 64ull * (q - gload < uint32_t > (&bd.chunk_base)), end = begin + 64u;
  uint64_t pos = begin + (word >> 2);
  if ((word & 3u) != kA) {
    // the rest of a code that started before
    const NdWalk r = nd_walk (nd_bits64 (B, begin), 0, word & 3u, 1u);
    if (r.count == 0)
      return;
    pos = begin + r.off;
  }
  const uint32_t ncb = (uint32_t) sb.hc * (uint32_t) sb.vc;
  const uint32_t *cbr = S.cb + (size_t) kNdCbWords * (size_t) sb.cb_base;
  NdGeo g = nd_geo (sb, c);
  uint32_t need = (uint32_t) g.w * (uint32_t) g.h;
  uint32_t qi = gload < uint32_t > (cbr + (size_t) kNdCbWords * c + 1) & 0xffu;
  uint32_t row = need ? n / (uint32_t) g.w : 0u, col = need ? n - row * (uint32_t) g.w : 0u;
  uint32_t longs = 0;
#pragma unroll 1
  for (;;) {
    // the next codeblock whose first value bit lies in this chunk
    bool any = true;
#pragma unroll 1
    while (n >= need) {
      if (++c >= ncb) {
        any = false;
        break;
      }
      // a head takes a bit wherever there is more than one codeblock: at most 64 of them lie in the chunk
      const uint64_t first = gload < uint32_t > (cbr + (size_t) kNdCbWords * c);
      if (first >= end) {
        any = false;
        break;
      }
      const uint32_t w1 = gload < uint32_t > (cbr + (size_t) kNdCbWords * c + 1);
      if (w1 & 0x100u)
        continue;               // a zero codeblock
      g = nd_geo (sb, c);
      need = (uint32_t) g.w * (uint32_t) g.h;
      if (need == 0)
        continue;
      if (gload < uint32_t > (cbr + (size_t) kNdCbWords * c + 2) == 0u) {
        any = false;
        break;
      }
      pos = first;
      qi = w1 & 0xffu;
      n = row = col = 0;
    }
    if (!any || pos >= end)
      break;
    const uint32_t m = nd_code (B, pos, longs, true);
    const size_t at = (size_t) (g.ymin + (int) row) * (size_t) sb.stride + (size_t) (g.xmin + (int) col) * sizeof (T);
    const uint32_t factor = kDevQuant.factor[qi], offset = pic.is_intra ? kDevQuant.off12[qi] : kDevQuant.off38[qi];
    gstore < T > ((T *) ((char *) sb.coeffs + at), dequant_one < T, ARITH > ((int32_t) (T) m, factor, offset));
    if (sb.quant)
      gstore < T > ((T *) ((char *) sb.quant + at), (T) m);
    n++;
    if (++col == (uint32_t) g.w) {
      col = 0;
      row++;
    }
  }
  if (longs)
    atomicAdd (&pic.result->long_codes, longs);
}

// ---- fill --------------------------------------------------------------------------------------------------------------

template < typename T >
__global__ __launch_bounds__ (64)
void nd_fill_kernel (const NdSubband * __restrict__ sbs, const NdPicture * __restrict__ pics, const NdScratch S)
{
  const NdSubband & sb = sbs[blockIdx.y];
  const NdPicture & pic = pics[sb.pic];
  if (gload < uint32_t > (&pic.result->error))
    return;
  const bool coded = gload < uint32_t > (&S.bands[blockIdx.y].flags) & 1u;
  const uint32_t *cbr = S.cb + (size_t) kNdCbWords * (size_t) sb.cb_base;
  const int npieces = sb.bh * sb.hc, lane = (int) threadIdx.x;
#pragma unroll 1
  for (int p = (int) blockIdx.x; p < npieces; p += (int) gridDim.x) {
    const int r = p / sb.hc, x = p - r * sb.hc;
    const int xmin = (x * sb.bw) / sb.hc, w = ((x + 1) * sb.bw) / sb.hc - xmin;
    int lo = 0;
    if (coded) {
      // the codeblock row that holds band row r: the last y with y bh / vc <= r
      const int y = (int) ((((int64_t) r + 1) * sb.vc - 1) / sb.bh);
      const int ymin = (y * sb.bh) / sb.vc;
      const uint32_t c = (uint32_t) y * (uint32_t) sb.hc + (uint32_t) x;
      if (!(gload < uint32_t > (cbr + (size_t) kNdCbWords * c + 1) & 0x100u)) {
        const int64_t ncoded = gload < uint32_t > (cbr + (size_t) kNdCbWords * c + 2);
        const int64_t n0 = (int64_t) (r - ymin) * w;
        lo = (int) max ((int64_t) 0, min ((int64_t) w, ncoded - n0));
      }
    }
    const size_t at = (size_t) r * (size_t) sb.stride;
    for (int i = lo + lane; i < w; i += 64) {
      gstore < T > ((T *) ((char *) sb.coeffs + at) + xmin + i, (T) 0);
      if (sb.quant)
        gstore < T > ((T *) ((char *) sb.quant + at) + xmin + i, (T) 0);
    }
  }
}

}                               // namespace

int
launch_noarith_decode (hipStream_t stream, const NdSubband * d_sbs, int nsbs, const NdPicture * d_pics, int npics,
    const NdScratch & S, int bpp, int lane_x, int fill_x, int stages)
{
  if (stages & 1)
    SCHRO_LAUNCH (nd_header_kernel, dim3 (npics), dim3 (64), 0, stream, d_sbs, d_pics, S);
  if (stages & 2)
    SCHRO_LAUNCH (nd_summary_kernel, dim3 (lane_x, npics), dim3 (kNdLaneThreads), 0, stream, d_pics, S);
  if (stages & 4)
    SCHRO_LAUNCH (nd_chain_kernel, dim3 (nsbs), dim3 (kNdChainThreads), 0, stream, d_sbs, d_pics, S);
  if (stages & 8) {
    if (bpp == 2) {
      SCHRO_LAUNCH ((nd_decode_kernel < int16_t, 1 >), dim3 (lane_x, npics), dim3 (kNdLaneThreads), 0, stream, d_sbs, d_pics, S);
      SCHRO_LAUNCH ((nd_fill_kernel < int16_t >), dim3 (fill_x, nsbs), dim3 (64), 0, stream, d_sbs, d_pics, S);
    } else {
      SCHRO_LAUNCH ((nd_decode_kernel < int32_t, 0 >), dim3 (lane_x, npics), dim3 (kNdLaneThreads), 0, stream, d_sbs, d_pics, S);
      SCHRO_LAUNCH ((nd_fill_kernel < int32_t >), dim3 (fill_x, nsbs), dim3 (64), 0, stream, d_sbs, d_pics, S);
    }
  }
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "noarith decode launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
