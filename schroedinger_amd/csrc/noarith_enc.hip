// noarith_enc.hip -- core-syntax transform data in the VLC parse codes, written on the device: the twin of
// schro_encoder_encode_transform_data (schroencoder.c:3462-3483) over schro_encoder_encode_subband_noarith (:4072-4192)
// without its quantiser call -- the quant planes are the input.
//
// Nothing carries over from one value to the next but the bit position, so the work is a count, a scan and a pack.  The
// unit is the PIECE: a codeblock's part of one sub-band row.  A sub-band of 1 x 1 codeblocks has one piece per row, so
// a whole 1920 x 1080 band spreads over 1080 workgroups; a piece is never cut, so there is no piece length to straddle.
//
//   na_count_kernel    a wave per piece (grid y: sub-band, grid x: up to kNaGridX workgroups that stride over the
//                      band's pieces): the bits of the piece's codes, the row sum schro_frame_data_is_zero takes (16-bit
//                      wrapped sum of 16-bit abs on s16, "any non-zero" on s32) and whether a value is truly non-zero.
//   na_layout_kernel   a workgroup per picture.  Per codeblock: its bits and the reference's zero test over its pieces;
//                      per band row: the test over the whole row (the sub-band's flag); an exclusive scan of the
//                      codeblocks' coded bits in stream order (kNaLayoutThreads threads, a run of codeblocks each); then
//                      thread 0 walks the serial chain of at most 57 sub-band headers -- each starts on a byte, its
//                      length is the payload's -- and writes the picture's result; last every piece gets its first bit.
//   na_clear_kernel    zeroes min (capacity, bytes) bytes of the output: what follows ORs into it.
//   na_pack_kernel     a wave per piece: the codes, an in-wave prefix sum of their lengths, bits OR-ed into a window of LDS
//                      words, whole words stored when the piece owns them, atomicOr where neighbours share a word.  Head
//                      units behind a band's pieces write the codeblocks' flag bits and the sub-band's header the same way.
//
// Bytes at and past the capacity are masked out of every store, so a picture that does not fit is cut, never overrun.

#include "schro_hip_internal.h"
#include "na_bits.h"

namespace schro {
namespace {

constexpr int kNaWinWords = 132;        // pack: 64 codes of up to 64 bits behind up to 31 carried bits, and slack for a code's third word

__device__ __forceinline__ NaOut
na_out (const NaPicture & pic)
{
  NaOut st;
  const uintptr_t addr = (uintptr_t) pic.out;
  st.wbase = (uint32_t *) (addr & ~(uintptr_t) 3);
  st.first_byte = (uint32_t) (addr & 3);
  st.end_byte = st.first_byte + pic.capacity;
  return st;
}

__device__ __forceinline__ int32_t
na_wave_sum (int32_t v)
{
#pragma unroll
  for (int d = 32; d; d >>= 1)
    v += __shfl_xor (v, d);
  return v;
}

__device__ __forceinline__ int32_t
na_load (const char *row, int i, int bpp)
{
  return bpp == 2 ? (int32_t) gload < int16_t > ((const int16_t *) row + i) : gload < int32_t > ((const int32_t *) row + i);
}

// ---- count ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (64)
void na_count_kernel (const NaSubband * __restrict__ sbs, const NaScratch S, const int bpp)
{
  const NaSubband & sb = sbs[blockIdx.y];
  const int lane = (int) threadIdx.x;
  const int bw = sb.bw, hc = sb.hc, npieces = sb.bh * hc;
#pragma unroll 1
  for (int p = (int) blockIdx.x; p < npieces; p += (int) gridDim.x) {
    const int r = p / hc, x = p - r * hc;
    const int xmin = (x * bw) / hc, xmax = ((x + 1) * bw) / hc;
    const char *row = (const char *) sb.base + (size_t) r * (size_t) sb.stride;
    int32_t bits = 0, sum = 0, nz = 0;
    for (int i = xmin + lane; i < xmax; i += 64) {
      const int32_t q = na_load (row, i, bpp);
      bits += na_sint_bits (q);
      // orc_accw over absw: 16-bit abs, 16-bit wrapped sum (abs (-32768) stays -32768, 0x8000 as a word)
      sum += bpp == 2 ? (int32_t) (na_mag (q) & 0xffffu) : (q != 0);
      nz |= q != 0;
    }
    bits = na_wave_sum (bits);
    sum = na_wave_sum (sum);
    nz = __ballot (nz) != 0;
    if (lane == 0) {
      const uint32_t s = bpp == 2 ? (uint32_t) sum & 0xffffu : (sum != 0);
      gstore < uint32_t > (S.bits + sb.piece_base + p, (uint32_t) bits);
      gstore < uint32_t > (S.info + sb.piece_base + p, s | ((uint32_t) nz << 16));
    }
  }
}

// ---- layout -----------------------------------------------------------------------------------------------------------

// the bits codeblock `cb` (of the call) of sub-band s takes in the payload
__device__ __forceinline__ uint32_t
na_coded_bits (const NaSubband & s, const NaScratch & S, int cb)
{
  const uint32_t fl = gload < uint32_t > (S.cb_flags + cb);
  const uint32_t zf = s.flags & 1, qo = (s.flags >> 1) & 1;
  if (zf && !(fl & 1u))
    return 1u;
  return zf + qo + gload < uint32_t > (S.cb_bits + cb);
}

__global__ __launch_bounds__ (kNaLayoutThreads)
void na_layout_kernel (const NaSubband * __restrict__ sbs, const NaPicture * __restrict__ pics, const NaScratch S, const int bpp)
{
  __shared__ NaSubband sb[kNaMaxSubbands];
  __shared__ uint32_t sb_ref[kNaMaxSubbands], sb_true[kNaMaxSubbands];  // the reference's test fails; truly non-zero
  __shared__ uint32_t part[kNaLayoutThreads];
  __shared__ uint32_t false_cb;
  const NaPicture & pic = pics[blockIdx.x];
  const int tid = (int) threadIdx.x, T = kNaLayoutThreads;
  const int nsb = pic.nsb, ncb = pic.ncb, cb_first = pic.cb_first;
  for (int k = tid; k < nsb * 16; k += T)
    ((uint32_t *) sb)[k] = gload < uint32_t > ((const uint32_t *) (sbs + pic.sb_first) + k);
  if (tid < kNaMaxSubbands)
    sb_ref[tid] = sb_true[tid] = 0;
  if (tid == 0)
    false_cb = 0;
  __syncthreads ();

  // per codeblock: the bits of its values, the reference's zero test over its row pieces, the true answer
  for (int c = tid; c < ncb; c += T) {
    int s = 0;
    while (s + 1 < nsb && sb[s + 1].cb_base - cb_first <= c)
      s++;
    const NaSubband & b = sb[s];
    const int k = c - (b.cb_base - cb_first), y = k / b.hc, x = k - y * b.hc;
    const int ymin = (y * b.bh) / b.vc, ymax = ((y + 1) * b.bh) / b.vc;
    uint32_t bits = 0, ref = 0, tru = 0;
    for (int r = ymin; r < ymax; r++) {
      const int p = b.piece_base + r * b.hc + x;
      const uint32_t i = gload < uint32_t > (S.info + p);
      bits += gload < uint32_t > (S.bits + p);
      ref |= (i & 0xffffu) != 0;
      tru |= i >> 16;
    }
    gstore < uint32_t > (S.cb_bits + cb_first + c, bits);
    gstore < uint32_t > (S.cb_flags + cb_first + c, ref | (tru << 1));
    if (tru)
      atomicOr (&sb_true[s], 1u);
  }
  // per band row: the same test over the sub-band's whole row
  for (int q = tid; q < pic.rows; q += T) {
    int s = 0;
    while (s + 1 < nsb && sb[s + 1].row_base <= q)
      s++;
    const NaSubband & b = sb[s];
    const int r = q - b.row_base;
    uint32_t acc = 0;
    for (int x = 0; x < b.hc; x++)
      acc += gload < uint32_t > (S.info + b.piece_base + r * b.hc + x) & 0xffffu;
    if (bpp == 2)
      acc &= 0xffffu;
    if (acc)
      atomicOr (&sb_ref[s], 1u);
  }
  __syncthreads ();

  // the exclusive scan of the codeblocks' coded bits in stream order: a run of codeblocks per thread
  const int run = (ncb + T - 1) / T;
  const int c0 = min (ncb, tid * run), c1 = min (ncb, c0 + run);
  uint32_t mine = 0;
  {
    int s = 0;
    for (int c = c0; c < c1; c++) {
      while (s + 1 < nsb && sb[s + 1].cb_base - cb_first <= c)
        s++;
      mine += na_coded_bits (sb[s], S, cb_first + c);
    }
  }
  part[tid] = mine;
  __syncthreads ();
  for (int d = 1; d < T; d <<= 1) {
    const uint32_t v = tid >= d ? part[tid - d] : 0u;
    __syncthreads ();
    part[tid] += v;
    __syncthreads ();
  }
  {
    uint32_t at = part[tid] - mine;
    int s = 0;
    for (int c = c0; c < c1; c++) {
      while (s + 1 < nsb && sb[s + 1].cb_base - cb_first <= c)
        s++;
      gstore < uint32_t > (S.cb_pos + cb_first + c, at);
      at += na_coded_bits (sb[s], S, cb_first + c);
    }
  }
  __syncthreads ();

  // the serial chain of sub-band headers: every sub-band starts on a byte
  if (tid == 0) {
    const uint32_t total = part[T - 1];
    uint32_t pos = 0, false_sb = 0;     // bytes
    for (int s = 0; s < nsb; s++) {
      const NaSubband & b = sb[s];
      const uint32_t p0 = gload < uint32_t > (S.cb_pos + b.cb_base);
      const uint32_t p1 = s + 1 < nsb ? gload < uint32_t > (S.cb_pos + sb[s + 1].cb_base) : total;
      const uint32_t length = sb_ref[s] ? (p1 - p0 + 7u) >> 3 : 0u;
      uint32_t bits = 0;
      gstore < uint32_t > (S.sb_at + pic.sb_first + s, 8u * pos);
      gstore < uint32_t > (S.sb_len + pic.sb_first + s, length);
      if (length == 0) {
        pos += 1;               // uint (0): one 1-bit, padded by the next sync; the byte offset had not moved (trap b)
      } else {
        int l0, l1;
        (void) na_uint_code (length, &l0);
        (void) na_uint_code ((uint32_t) b.quant_index, &l1);
        const uint32_t header = (uint32_t) (l0 + l1 + 7) >> 3;
        bits = 8u * (header + length);
        pos += header + length;
      }
      false_sb += !sb_ref[s] && sb_true[s];
      gstore < uint32_t > (&pic.result->subband_bits[b.comp][b.index], bits);
    }
    gstore < uint32_t > (&pic.result->bytes, pos);
    gstore < uint32_t > (&pic.result->overrun, pos > pic.capacity ? 1u : 0u);
    gstore < uint32_t > (&pic.result->false_zero_subbands, false_sb);
  }
  __syncthreads ();

  // every codeblock's and every piece's first bit
  for (int c = tid; c < ncb; c += T) {
    int s = 0;
    while (s + 1 < nsb && sb[s + 1].cb_base - cb_first <= c)
      s++;
    const NaSubband & b = sb[s];
    const uint32_t length = gload < uint32_t > (S.sb_len + pic.sb_first + s);
    if (length == 0)
      continue;                 // nothing of the sub-band but its one bit is written
    int l0, l1;
    (void) na_uint_code (length, &l0);
    (void) na_uint_code ((uint32_t) b.quant_index, &l1);
    const uint32_t payload = gload < uint32_t > (S.sb_at + pic.sb_first + s) + 8u * ((uint32_t) (l0 + l1 + 7) >> 3);
    const uint32_t fl = gload < uint32_t > (S.cb_flags + cb_first + c);
    const uint32_t zf = b.flags & 1, qo = (b.flags >> 1) & 1;
    const bool zero = zf && !(fl & 1u);
    const uint32_t at = payload + gload < uint32_t > (S.cb_pos + cb_first + c) - gload < uint32_t > (S.cb_pos + b.cb_base);
    gstore < uint32_t > (S.cb_at + cb_first + c, at);
    if (zero && (fl & 2u))
      atomicAdd (&false_cb, 1u);
    const int k = c - (b.cb_base - cb_first), y = k / b.hc, x = k - y * b.hc;
    const int ymin = (y * b.bh) / b.vc, ymax = ((y + 1) * b.bh) / b.vc;
    uint32_t first = at + zf + qo;
    for (int r = ymin; r < ymax; r++) {
      const int p = b.piece_base + r * b.hc + x;
      gstore < uint32_t > (S.start + p, zero ? kNaNone : first);
      first += gload < uint32_t > (S.bits + p);
    }
  }
  __syncthreads ();
  if (tid == 0)
    gstore < uint32_t > (&pic.result->false_zero_codeblocks, false_cb);
}

// ---- clear ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (256)
void na_clear_kernel (const NaPicture * __restrict__ pics)
{
  const NaPicture & pic = pics[blockIdx.y];
  NaOut st = na_out (pic);
  st.end_byte = st.first_byte + min (pic.capacity, gload < uint32_t > (&pic.result->bytes));
  const uint32_t w0 = 4u * ((uint32_t) blockIdx.x * 256u + (uint32_t) threadIdx.x);
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t w = w0 + k, m = na_mask (st, w);
    if (m == 0xffffffffu) {
      gstore < uint32_t > (st.wbase + w, 0u);
    } else if (m) {
#pragma unroll
      for (uint32_t j = 0; j < 4; j++)
        if (m & (0xff000000u >> (8u * j)))
          gstore < uint8_t > ((uint8_t *) (st.wbase + w) + j, (uint8_t) 0);
    }
  }
}

// ---- pack -------------------------------------------------------------------------------------------------------------

struct NaPiece {
  uint32_t begin, end;          // the piece's bits, from wbase
  uint32_t pos;                 // bits written so far
};

// every lane's code (len 0: none) behind the bits written so far
__device__ __forceinline__ void
na_emit (const NaOut & st, NaPiece & pc, uint32_t * win, uint64_t code, int len, int lane)
{
  uint32_t incl = (uint32_t) len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t) __shfl_up ((int) incl, d);
    incl += lane >= d ? o : 0u;
  }
  const uint32_t total = (uint32_t) __shfl ((int) incl, 63);
  const uint32_t w0 = pc.pos >> 5;
  if (len) {
    const uint32_t rel = pc.pos + incl - (uint32_t) len - (w0 << 5), sh = rel & 31u, w = rel >> 5;
    const uint64_t v = code << (64 - len);
    const uint32_t hi = (uint32_t) (v >> 32), lo = (uint32_t) v;
    const uint32_t a = hi >> sh, b = sh ? (hi << (32u - sh)) | (lo >> sh) : lo, c = sh ? lo << (32u - sh) : 0u;
    if (a)
      atomicOr (&win[w], a);
    if (b)
      atomicOr (&win[w + 1], b);
    if (c)
      atomicOr (&win[w + 2], c);
  }
  __syncthreads ();
  const uint32_t pos1 = pc.pos + total;
  const uint32_t nfull = (pos1 >> 5) - w0;      // <= 129 whole words
  const uint32_t carry = win[nfull];
  for (uint32_t k = (uint32_t) lane; k < nfull; k += 64u) {
    const uint32_t w = w0 + k, value = win[k];
    // a word all of whose bits are this piece's is stored; one shared with a neighbour is OR-ed into the cleared output
    if (32u * w >= pc.begin && 32u * w + 32u <= pc.end && na_mask (st, w) == 0xffffffffu)
      gstore < uint32_t > (st.wbase + w, __builtin_bswap32 (value));
    else
      na_or_word (st, w, value);
  }
  __syncthreads ();
  for (int k = lane; k < kNaWinWords; k += 64)
    win[k] = 0;
  __syncthreads ();
  if (lane == 0)
    win[0] = carry;
  __syncthreads ();
  pc.pos = pos1;
}

__global__ __launch_bounds__ (64)
void na_pack_kernel (const NaSubband * __restrict__ sbs, const NaPicture * __restrict__ pics, const int *__restrict__ sb_pic,
    const NaScratch S, const int bpp)
{
  __shared__ uint32_t win[kNaWinWords];
  const int g = (int) blockIdx.y;
  const NaSubband & sb = sbs[g];
  const NaPicture & pic = pics[sb_pic[g]];
  const NaOut st = na_out (pic);
  const int lane = (int) threadIdx.x;
  const int bw = sb.bw, hc = sb.hc, npieces = sb.bh * hc, ncb = hc * sb.vc;
  const int nunits = npieces + (ncb + 63) / 64;
  const uint32_t length = gload < uint32_t > (S.sb_len + g);
  const uint32_t origin = 8u * st.first_byte;
#pragma unroll 1
  for (int u = (int) blockIdx.x; u < nunits; u += (int) gridDim.x) {
    if (u >= npieces) {
      // a head unit: the flag bits of 64 codeblocks; the first one also writes the sub-band's header
      const int h = u - npieces, k = h * 64 + lane;
      if (length && k < ncb) {
        const uint32_t fl = gload < uint32_t > (S.cb_flags + sb.cb_base + k);
        const uint32_t at = gload < uint32_t > (S.cb_at + sb.cb_base + k);
        const int zf = sb.flags & 1, qo = (sb.flags >> 1) & 1;
        const bool zero = zf && !(fl & 1u);
        // bit (zero), then sint (0) -- one 1-bit -- in front of a codeblock that is written
        if (zero)
          na_or_bits (st, origin + at, 1u, 1);
        else
          na_or_bits (st, origin + at, (uint64_t) qo, zf + qo);
      }
      if (h == 0 && lane == 0) {
        const uint32_t at = origin + gload < uint32_t > (S.sb_at + g);
        int l0, l1;
        const uint64_t c0 = na_uint_code (length, &l0);
        na_or_bits (st, at, c0, l0);
        if (length) {
          const uint64_t c1 = na_uint_code ((uint32_t) sb.quant_index, &l1);
          na_or_bits (st, at + (uint32_t) l0, c1, l1);
        }
      }
      continue;
    }
    if (!length)
      continue;
    const uint32_t start = gload < uint32_t > (S.start + sb.piece_base + u);
    if (start == kNaNone)
      continue;
    const int r = u / hc, x = u - r * hc;
    const int xmin = (x * bw) / hc, xmax = ((x + 1) * bw) / hc;
    if (xmax <= xmin)
      continue;
    const char *row = (const char *) sb.base + (size_t) r * (size_t) sb.stride;
    NaPiece pc;
    pc.begin = pc.pos = origin + start;
    pc.end = pc.begin + gload < uint32_t > (S.bits + sb.piece_base + u);
    __syncthreads ();
    for (int k = lane; k < kNaWinWords; k += 64)
      win[k] = 0;
    __syncthreads ();
#pragma unroll 1
    for (int i0 = xmin; i0 < xmax; i0 += 64) {
      const int i = i0 + lane;
      int len = 0;
      uint64_t code = 0;
      if (i < xmax)
        code = na_sint_code (na_load (row, i, bpp), &len);
      na_emit (st, pc, win, code, len, lane);
    }
    // the bits of the last, partial word
    if (lane == 0 && (pc.pos & 31u))
      na_or_word (st, pc.pos >> 5, win[0]);
  }
}

// schro_hip_noarith_encode_chosen_batch: the quant index of every sub-band's header from the picture's chosen indices on
// the device ([3][19] int32); a value outside 0 .. 60 is clamped into range and counted
__global__ __launch_bounds__ (64)
void na_resolve_kernel (NaSubband * __restrict__ sbs, int nsbs, const int *__restrict__ sb_pic, const int32_t * const *__restrict__ chosen,
    uint32_t * clamped)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nsbs)
    return;
  const int32_t q = chosen[sb_pic[t]][sbs[t].comp * SCHRO_HIP_NOARITH_MAX_SUBBANDS + sbs[t].index];
  if (q < 0 || q > 60)
    __hip_atomic_fetch_add (clamped, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  sbs[t].quant_index = q < 0 ? 0 : (q > 60 ? 60 : q);
}

}                               // namespace

int
launch_noarith_resolve (hipStream_t stream, NaSubband * d_sbs, int nsbs, const int *d_sb_pic, const int32_t * const *d_chosen, uint32_t * clamped)
{
  SCHRO_LAUNCH (na_resolve_kernel, dim3 (div_up (nsbs, 64)), dim3 (64), 0, stream, d_sbs, nsbs, d_sb_pic, d_chosen, clamped);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "noarith resolve launch: %s", hipGetErrorString (e));
  return 0;
}

int
launch_noarith_encode (hipStream_t stream, const NaSubband * d_sbs, int nsbs, const NaPicture * d_pics, int npics,
    const NaScratch & S, int bpp, int grid_x, int clear_x, int stages)
{
  // behind the pictures: the picture of every sub-band
  const int *d_sb_pic = (const int *) (d_pics + npics);
  if (stages & 1)
    SCHRO_LAUNCH (na_count_kernel, dim3 (grid_x, nsbs), dim3 (64), 0, stream, d_sbs, S, bpp);
  if (stages & 2)
    SCHRO_LAUNCH (na_layout_kernel, dim3 (npics), dim3 (kNaLayoutThreads), 0, stream, d_sbs, d_pics, S, bpp);
  if (stages & 4) {
    SCHRO_LAUNCH (na_clear_kernel, dim3 (clear_x, npics), dim3 (256), 0, stream, d_pics);
    SCHRO_LAUNCH (na_pack_kernel, dim3 (grid_x, nsbs), dim3 (64), 0, stream, d_sbs, d_pics, d_sb_pic, S, bpp);
  }
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "noarith encode launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
