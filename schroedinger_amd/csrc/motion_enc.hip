// motion_enc.hip -- the motion data of a noarith (VLC) picture, written on the device: the twin of what
// schro_encoder_encode_picture appends between the prediction parameters and the transform parameters
// (schroencoder.c:2505-2515) -- schro_encoder_encode_superblock_split, _prediction_modes, _vector_data (ref, xy) and
// _dc_data (comp), :2841-3142, in their params->is_noarith branches -- over the predictors of schromotion.c:163-430.
//
// The encoder's predictions read the neighbours' RECORDS, not decoded state, so nothing carries over from one unit to the
// next but the bit position: the work is a count, a scan and a pack, as in noarith_enc.hip.  One lane per block; the 16
// lanes of a DPP row are one superblock in raster order of its blocks, which is the stream order of the units that exist
// for its split (steps of 4 >> split from the top-left block); a wave holds four consecutive superblocks of the picture's
// raster order.
//
//   me_count_kernel    every lane: its record, its three neighbours' flags, dx and dy words, the bits it contributes to
//                      each of the nine sections (0 where the unit does not exist); a row reduction gives the nine totals
//                      and unit counts of the superblock, and what schro_motion_verify and the two asserts would say.
//   me_layout_kernel   a workgroup per picture: the exclusive scans of the superblocks' totals per section (a run of
//                      superblocks per thread), then thread 0 walks the serial chain of 7 or 9 section headers -- each
//                      starts on a byte, its length is the payload's -- and writes the result; last every superblock
//                      gets its first bit in every section.
//   me_clear_kernel    zeroes min (capacity, bytes) bytes of the output: what follows ORs into it.
//   me_pack_kernel     the same lanes, the codes again, an in-row prefix of their lengths, bits OR-ed into one LDS window
//                      per row and section, the windows' words OR-ed into the output under the byte masks of na_bits.h.
//
// Bytes at and past the capacity are masked out of every store, so a picture that does not fit is cut, never overrun.
// Whatever the records hold, a code is the sint code of a difference of two values in int16 range: at most 34 bits.

#include "motion_common.h"
#include "na_bits.h"

namespace schro {
namespace {

constexpr int kMeWinWords = 20; // pack: 16 codes of up to 34 bits behind up to 31 bits of the row's first word, and slack for a code's third word

struct MeRec {
  uint32_t flags, dx, dy;
};

// the three neighbours of block (x, y) as vector_prediction's source of records
struct MeNeighbours {
  int x, y;
  MeRec left, above, diag;
  __device__ __forceinline__ bool operator () (int xx, int yy, int mode, int *vx, int *vy) const
  {
    const MeRec & r = yy == y ? left : (xx == x ? above : diag);
    return mv_predicts (r.flags, r.dx, r.dy, mode, vx, vy);
  }
};

__device__ __forceinline__ MeRec
me_load (const uint8_t * field, int nbx, int x, int y)
{
  MeRec r;
  GlobalRecords { field, nbx }.raw (x, y, &r.flags, &r.dx, &r.dy);
  return r;
}

// dc[i] of a record: the union's first three int16
__device__ __forceinline__ int
me_dc (const MeRec & r, int i)
{
  return i == 0 ? (int16_t) r.dx : i == 1 ? (int16_t) (r.dx >> 16) : (int16_t) r.dy;
}

// what one lane contributes
struct MeLane {
  uint64_t code[kMeSections];
  int len[kMeSections];         // 0: the section has no unit here
  uint32_t unverified, asserted;
  int sb;                       // its superblock in the picture, -1: none
  uint32_t index;               // its block's raster index
};

__device__ __forceinline__ int
me_split (const uint8_t * field, int nbx, int x, int y)
{
  return (int) ((gload < uint32_t > (mv_record (field, nbx, x, y) + kMvFlags) >> 3) & 3u);
}

// Every lane of the wave comes here (the verify test shuffles within rows).
__device__ __forceinline__ void
me_lane (const MePicture & pic, int wave, int lane, MeLane & u)
{
  const int nbx = pic.nbx, nsbx = nbx >> 2, nsb = nsbx * (pic.nby >> 2);
  const int r = lane & 15, sb = wave * 4 + (lane >> 4);
  const bool valid = sb < nsb;
  const int sy = valid ? sb / nsbx : 0, sx = valid ? sb - sy * nsbx : 0;
  const int x = 4 * sx + (r & 3), y = 4 * sy + (r >> 2);
  const uint8_t *field = pic.motion;
#pragma unroll
  for (int s = 0; s < kMeSections; s++)
    u.code[s] = 0, u.len[s] = 0;
  u.unverified = u.asserted = 0;
  u.sb = valid ? sb : -1;
  u.index = (uint32_t) (y * nbx + x);

  uint32_t w[kMvDwords];
#pragma unroll
  for (int k = 0; k < kMvDwords; k++)
    w[k] = valid ? gload < uint32_t > (mv_record (field, nbx, x, y) + 4 * k) : 0u;
  const MeRec own = { w[0], w[kMvDx / 4], w[kMvDy / 4] };
  const int mode = (int) (own.flags & 3u), ug = (int) ((own.flags >> 2) & 1u), split = (int) ((own.flags >> 3) & 3u);
  const int sbsplit = __shfl (split, 0, 16);

  // schro_motion_verify (schromotion.c:441-525): the split, the copies, the DC range, the mode, the global flag
  {
    const int origin = sbsplit == 0 ? 0 : sbsplit == 1 ? (r & 10) : r;
    bool bad = split != sbsplit;
#pragma unroll
    for (int k = 0; k < kMvDwords; k++)
      bad |= (uint32_t) __shfl ((int) w[k], origin, 16) != w[k];
    if (mode == 0)
#pragma unroll
      for (int i = 0; i < 3; i++)
        bad |= me_dc (own, i) < -128 || me_dc (own, i) > 127;
    bad |= mode >= 2 && pic.num_refs < 2;
    bad |= ug && !pic.have_global;
    u.unverified = valid && bad ? 1u : 0u;
  }
  if (!valid)
    return;

  // the superblock's split residual (schro_motion_split_prediction, :371-399, reads records 4 away)
  if (r == 0) {
    int pred = 0;
    if (y == 0) {
      if (x > 0)
        pred = me_split (field, nbx, x - 4, 0);
    } else if (x == 0) {
      pred = me_split (field, nbx, 0, y - 4);
    } else {
      pred = (me_split (field, nbx, x, y - 4) + me_split (field, nbx, x - 4, y) + me_split (field, nbx, x - 4, y - 4) + 1) / 3;
    }
    u.code[0] = na_uint_code ((uint32_t) ((split - pred + 3) % 3), &u.len[0]);
    u.asserted += split == 3;   // SCHRO_ASSERT (mv->split < 3): coded as split 2, where the reference would not end
  }
  const int step = 4 >> min (sbsplit, 2);
  if (((r | (r >> 2)) & 3 & (step - 1)) != 0)
    return;                     // no unit here for this split

  MeNeighbours nb;
  nb.x = x, nb.y = y;
  nb.left = nb.above = nb.diag = MeRec { 0u, 0u, 0u };
  if (x > 0)
    nb.left = me_load (field, nbx, x - 1, y);
  if (y > 0)
    nb.above = me_load (field, nbx, x, y - 1);
  if (x > 0 && y > 0)
    nb.diag = me_load (field, nbx, x - 1, y - 1);

  // prediction modes (:2906-2954; schro_motion_get_mode_prediction, schro_motion_get_global_prediction)
  {
    const uint32_t a = nb.left.flags, b = nb.above.flags, c = nb.diag.flags;
    // at an edge the one neighbour there is; inside the majority of three, bit by bit
    const uint32_t maj = y == 0 ? a : x == 0 ? b : (a & b) | (b & c) | (c & a);
    const int res = mode ^ (int) (maj & 3u);
    uint64_t code = (uint64_t) (res & 1);
    int len = 1;
    if (pic.num_refs > 1)
      code = (code << 1) | (uint64_t) (res >> 1), len++;
    if (mode != 0) {
      if (pic.have_global)
        code = (code << 1) | (uint64_t) (ug ^ (int) ((maj >> 2) & 1u)), len++;
      else
        u.asserted += ug;       // SCHRO_ASSERT (mv->using_global == FALSE)
    }
    u.code[1] = code, u.len[1] = len;
  }

  // vectors (:3010-3047): present iff the mode names the reference and the block is not global
#pragma unroll
  for (int ref = 0; ref < 2; ref++)
    if (ref < pic.num_refs && (mode & (1 << ref)) && !ug) {
      int px, py;
      vector_prediction (nb, x, y, 1 << ref, &px, &py);
      const int vx = (int16_t) (own.dx >> (16 * ref)), vy = (int16_t) (own.dy >> (16 * ref));
      u.code[2 + 2 * ref] = na_sint_code (vx - px, &u.len[2 + 2 * ref]);
      u.code[3 + 2 * ref] = na_sint_code (vy - py, &u.len[3 + 2 * ref]);
    }

  // DC (:3080-3126; schro_motion_dc_prediction, :163-210): the neighbours of mode 0, whatever their global flag
  if (mode == 0) {
    const bool pl = x > 0 && (nb.left.flags & 3u) == 0, pa = y > 0 && (nb.above.flags & 3u) == 0;
    const bool pd = x > 0 && y > 0 && (nb.diag.flags & 3u) == 0;
    const int n = (int) pl + (int) pa + (int) pd;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int sum = (pl ? me_dc (nb.left, i) : 0) + (pa ? me_dc (nb.above, i) : 0) + (pd ? me_dc (nb.diag, i) : 0);
      // n == 1: (short) sum; 2: (sum + 1) >> 1; 3: schro_divide3 (sum + 1) = ((a) * 21845 + 10922) >> 16, an arithmetic shift
      const int pred = n == 0 ? 0 : n == 1 ? (int) (int16_t) sum : n == 2 ? (sum + 1) >> 1 : ((sum + 1) * 21845 + 10922) >> 16;
      u.code[6 + i] = na_sint_code (me_dc (own, i) - pred, &u.len[6 + i]);
    }
  }
}

// three sections' lengths (each at most 16 x 34 in a row) in one word
__device__ __forceinline__ uint32_t
me_pack3 (const int *len)
{
  return (uint32_t) len[0] | ((uint32_t) len[1] << 10) | ((uint32_t) len[2] << 20);
}

__device__ __forceinline__ uint32_t
me_row_sum (uint32_t v)
{
#pragma unroll
  for (int d = 8; d; d >>= 1)
    v += (uint32_t) __shfl_xor ((int) v, d, 16);
  return v;
}

// ---- count ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (64)
void me_count_kernel (const MePicture * __restrict__ pics, uint32_t * __restrict__ scratch)
{
  const MePicture & pic = pics[blockIdx.y];
  const int lane = (int) threadIdx.x;
  const int nsb = (pic.nbx >> 2) * (pic.nby >> 2);
  if ((int) blockIdx.x * 4 >= nsb)
    return;
  MeLane u;
  me_lane (pic, (int) blockIdx.x, lane, u);
  uint32_t bits[3], units[2] = { 0u, 0u };
#pragma unroll
  for (int k = 0; k < 3; k++)
    bits[k] = me_row_sum (me_pack3 (u.len + 3 * k));
#pragma unroll
  for (int s = 0; s < kMeSections; s++)
    units[s / 6] |= (u.len[s] ? 1u : 0u) << (5 * (s % 6));
  // behind the three unit counts of the second word: the blocks verify rejects (at most 16) and the asserts (at most 17)
  units[1] |= (u.unverified << 15) | (u.asserted << 20);
  units[0] = me_row_sum (units[0]);
  units[1] = me_row_sum (units[1]);
  uint32_t first = u.unverified ? u.index : 0xffffffffu;
#pragma unroll
  for (int d = 8; d; d >>= 1)
    first = min (first, (uint32_t) __shfl_xor ((int) first, d, 16));
  if ((lane & 15) == 0 && u.sb >= 0) {
    uint32_t *o = scratch + (size_t) (pic.sb_first + u.sb) * kMeSbWords;
#pragma unroll
    for (int s = 0; s < kMeSections; s++) {
      gstore < uint32_t > (o + kMeBits + s, (bits[s / 3] >> (10 * (s % 3))) & 1023u);
      gstore < uint32_t > (o + kMeUnits + s, (units[s / 6] >> (5 * (s % 6))) & 31u);
    }
    gstore < uint32_t > (o + kMeUnverified, (units[1] >> 15) & 31u);
    gstore < uint32_t > (o + kMeFirst, first);
    gstore < uint32_t > (o + kMeAsserted, (units[1] >> 20) & 31u);
  }
}

// ---- layout -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__ (kMeLayoutThreads)
void me_layout_kernel (const MePicture * __restrict__ pics, uint32_t * __restrict__ scratch, uint32_t * __restrict__ sections)
{
  __shared__ uint32_t part[kMeSections][kMeLayoutThreads];
  __shared__ uint32_t tot_units[kMeSections], tot_unverified, tot_first, tot_asserted;
  __shared__ uint32_t payload_at[kMeSections];
  const MePicture & pic = pics[blockIdx.x];
  const int tid = (int) threadIdx.x, T = kMeLayoutThreads;
  const int nsb = (pic.nbx >> 2) * (pic.nby >> 2);
  uint32_t *sbw = scratch + (size_t) pic.sb_first * kMeSbWords;
  if (tid < kMeSections)
    tot_units[tid] = 0;
  if (tid == 0)
    tot_unverified = tot_asserted = 0, tot_first = 0xffffffffu;
  __syncthreads ();

  // a run of superblocks per thread
  const int run = (nsb + T - 1) / T;
  const int c0 = min (nsb, tid * run), c1 = min (nsb, c0 + run);
  uint32_t mine[kMeSections], units[kMeSections], unverified = 0, first = 0xffffffffu, asserted = 0;
#pragma unroll
  for (int s = 0; s < kMeSections; s++)
    mine[s] = units[s] = 0;
  for (int c = c0; c < c1; c++) {
    const uint32_t *o = sbw + (size_t) c * kMeSbWords;
#pragma unroll
    for (int s = 0; s < kMeSections; s++) {
      mine[s] += gload < uint32_t > (o + kMeBits + s);
      units[s] += gload < uint32_t > (o + kMeUnits + s);
    }
    unverified += gload < uint32_t > (o + kMeUnverified);
    first = min (first, gload < uint32_t > (o + kMeFirst));
    asserted += gload < uint32_t > (o + kMeAsserted);
  }
  if (c1 > c0) {
#pragma unroll
    for (int s = 0; s < kMeSections; s++)
      if (units[s])
        atomicAdd (&tot_units[s], units[s]);
    if (unverified) {
      atomicAdd (&tot_unverified, unverified);
      atomicMin (&tot_first, first);
    }
    if (asserted)
      atomicAdd (&tot_asserted, asserted);
  }
  // the inclusive scan of the runs' bits, all sections at once
#pragma unroll
  for (int s = 0; s < kMeSections; s++)
    part[s][tid] = mine[s];
  __syncthreads ();
  for (int d = 1; d < T; d <<= 1) {
    uint32_t v[kMeSections];
#pragma unroll
    for (int s = 0; s < kMeSections; s++)
      v[s] = tid >= d ? part[s][tid - d] : 0u;
    __syncthreads ();
#pragma unroll
    for (int s = 0; s < kMeSections; s++)
      part[s][tid] += v[s];
    __syncthreads ();
  }

  // the serial chain of section headers: every section starts on a byte
  if (tid == 0) {
    uint32_t *sec = sections + (size_t) blockIdx.x * 2 * kMeSections;
    uint32_t pos = 0;           // bytes
    for (int s = 0; s < kMeSections; s++) {
      const bool absent = pic.num_refs < 2 && (s == 4 || s == 5);
      const uint32_t length = absent ? 0u : (part[s][T - 1] + 7u) >> 3;
      int l0;
      (void) na_uint_code (length, &l0);
      const uint32_t header = (uint32_t) (l0 + 7) >> 3;
      gstore < uint32_t > (sec + s, absent ? kNaNone : 8u * pos);
      gstore < uint32_t > (sec + kMeSections + s, length);
      payload_at[s] = 8u * (pos + header);
      if (!absent)
        pos += header + length;
      gstore < uint32_t > (&pic.result->section_bytes[s], length);
      gstore < uint32_t > (&pic.result->section_units[s], absent ? 0u : tot_units[s]);
    }
    gstore < uint32_t > (&pic.result->bytes, pos);
    gstore < uint32_t > (&pic.result->overrun, pos > pic.capacity ? 1u : 0u);
    gstore < uint32_t > (&pic.result->asserted, tot_asserted);
    gstore < uint32_t > (&pic.result->unverified, tot_unverified);
    gstore < int32_t > (&pic.result->first_unverified, tot_unverified ? (int32_t) tot_first : -1);
  }
  __syncthreads ();

  // every superblock's first bit in every section
  uint32_t at[kMeSections];
#pragma unroll
  for (int s = 0; s < kMeSections; s++)
    at[s] = payload_at[s] + part[s][tid] - mine[s];
  for (int c = c0; c < c1; c++) {
    uint32_t *o = sbw + (size_t) c * kMeSbWords;
#pragma unroll
    for (int s = 0; s < kMeSections; s++) {
      gstore < uint32_t > (o + kMePos + s, at[s]);
      at[s] += gload < uint32_t > (o + kMeBits + s);
    }
  }
}

// ---- clear ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ NaOut
me_out (const MePicture & pic, uint32_t bytes)
{
  NaOut st;
  const uintptr_t addr = (uintptr_t) pic.out;
  st.wbase = (uint32_t *) (addr & ~(uintptr_t) 3);
  st.first_byte = (uint32_t) (addr & 3);
  st.end_byte = st.first_byte + bytes;
  return st;
}

__global__ __launch_bounds__ (256)
void me_clear_kernel (const MePicture * __restrict__ pics)
{
  const MePicture & pic = pics[blockIdx.y];
  const NaOut st = me_out (pic, min (pic.capacity, gload < uint32_t > (&pic.result->bytes)));
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

__global__ __launch_bounds__ (64)
void me_pack_kernel (const MePicture * __restrict__ pics, const uint32_t * __restrict__ scratch, const uint32_t * __restrict__ sections)
{
  __shared__ uint32_t win[4][kMeSections][kMeWinWords];
  const MePicture & pic = pics[blockIdx.y];
  const int lane = (int) threadIdx.x;
  const int nsb = (pic.nbx >> 2) * (pic.nby >> 2);
  if ((int) blockIdx.x * 4 >= nsb)
    return;
  const NaOut st = me_out (pic, pic.capacity);
  const uint32_t origin = 8u * st.first_byte;
  uint32_t *flat = &win[0][0][0];
  for (int k = lane; k < 4 * kMeSections * kMeWinWords; k += 64)
    flat[k] = 0;
  __syncthreads ();

  MeLane u;
  me_lane (pic, (int) blockIdx.x, lane, u);
  // where the units before this one in the row end: an inclusive prefix over the row's lanes, three sections a word
  uint32_t own[3], incl[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    own[k] = incl[k] = me_pack3 (u.len + 3 * k);
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const uint32_t o = (uint32_t) __shfl_up ((int) incl[k], d, 16);
      incl[k] += (lane & 15) >= d ? o : 0u;
    }
  }
  const int row = lane >> 4;
  if (u.sb >= 0) {
    const uint32_t *o = scratch + (size_t) (pic.sb_first + u.sb) * kMeSbWords + kMePos;
#pragma unroll
    for (int s = 0; s < kMeSections; s++) {
      const int len = u.len[s];
      if (len) {
        const uint32_t before = ((incl[s / 3] - own[s / 3]) >> (10 * (s % 3))) & 1023u;
        const uint32_t rel = ((origin + gload < uint32_t > (o + s)) & 31u) + before, sh = rel & 31u, w = rel >> 5;
        const uint64_t v = u.code[s] << (64 - len);
        const uint32_t hi = (uint32_t) (v >> 32), lo = (uint32_t) v;
        const uint32_t a = hi >> sh, b = sh ? (hi << (32u - sh)) | (lo >> sh) : lo, c = sh ? lo << (32u - sh) : 0u;
        // w + 2 <= (31 + 15 * 34) / 32 + 2 < kMeWinWords
        if (a)
          atomicOr (&win[row][s][w], a);
        if (b)
          atomicOr (&win[row][s][w + 1], b);
        if (c)
          atomicOr (&win[row][s][w + 2], c);
      }
    }
  }
  __syncthreads ();
  // the windows' words: neighbours in the stream share a word, so every one is OR-ed into the cleared output
  for (int k = lane; k < 4 * kMeSections * kMeWinWords; k += 64) {
    const uint32_t value = flat[k];
    if (value) {
      const int rw = k / (kMeSections * kMeWinWords), s = (k / kMeWinWords) % kMeSections, w = k % kMeWinWords;
      const uint32_t pos = gload < uint32_t > (scratch + (size_t) (pic.sb_first + (int) blockIdx.x * 4 + rw) * kMeSbWords + kMePos + s);
      na_or_word (st, ((origin + pos) >> 5) + (uint32_t) w, value);
    }
  }
  // the section headers: uint (payload bytes)
  if (blockIdx.x == 0 && lane < kMeSections) {
    const uint32_t *sec = sections + (size_t) blockIdx.y * 2 * kMeSections;
    const uint32_t at = gload < uint32_t > (sec + lane);
    if (at != kNaNone) {
      int l0;
      const uint64_t c0 = na_uint_code (gload < uint32_t > (sec + kMeSections + lane), &l0);
      na_or_bits (st, origin + at, c0, l0);
    }
  }
}

}                               // namespace

int
launch_motion_encode (hipStream_t stream, const MePicture * d_pics, int npics, uint32_t * scratch, int total_sbs, int waves_x, int clear_x,
    int stages)
{
  uint32_t *sections = scratch + (size_t) total_sbs * kMeSbWords;
  if (stages & 1)
    SCHRO_LAUNCH (me_count_kernel, dim3 (waves_x, npics), dim3 (64), 0, stream, d_pics, scratch);
  if (stages & 2)
    SCHRO_LAUNCH (me_layout_kernel, dim3 (npics), dim3 (kMeLayoutThreads), 0, stream, d_pics, scratch, sections);
  if (stages & 4)
    SCHRO_LAUNCH (me_clear_kernel, dim3 (clear_x, npics), dim3 (256), 0, stream, d_pics);
  if (stages & 8)
    SCHRO_LAUNCH (me_pack_kernel, dim3 (waves_x, npics), dim3 (64), 0, stream, d_pics, scratch, sections);
  hipError_t e = hipGetLastError ();
  if (e != hipSuccess)
    return set_error (SCHRO_HIP_EDEVICE, "motion encode launch: %s", hipGetErrorString (e));
  return 0;
}

}                               // namespace schro
