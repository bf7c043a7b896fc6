// schro_hip_internal.h -- shared between the HIP translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdint>
#include <cstddef>
#include <vector>

#include "schro_hip.h"

// The device-free build of the host code for the sanitizers (schro_hip_dry.h: test infrastructure, never shipped): the
// HIP runtime's entry points become host stand-ins and launches are dropped.
#ifdef SCHRO_HIP_DRY
#include "schro_hip_dry.h"
#endif

// Switches that force one of the library's kernels where another would be chosen (the tests' second
// formulations, A/B runs) and the measured-slower forms they select live in the EXPERIMENTS build only
// (libschro_hip_exp.so: make exp, -DSCHRO_HIP_EXPERIMENTS; tests/test_gpu_experiments.py runs it in child
// processes).  The product library reads no SCHRO_HIP_* variable but SCHRO_HIP_DEBUG.
#ifdef SCHRO_HIP_EXPERIMENTS
#define SCHRO_ENV(name) getenv (name)
#else
#define SCHRO_ENV(name) ((const char *) nullptr)
#endif

namespace schro {

int set_error (int code, const char *fmt, ...);
// the same, but never aborts: an answer the caller routes on (SCHRO_HIP_ENEEDS_RESIDUAL), not a trapped assertion
int set_status (int code, const char *fmt, ...);

static inline int
div_up (int a, int b)
{
  return (a + b - 1) / b;
}

static inline size_t
round_up (size_t a, size_t b)
{
  return (a + b - 1) / b * b;
}

#define SCHRO_HIP_CHECK(expr)                                                  \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      return schro::set_error (SCHRO_HIP_EDEVICE, "%s:%d: %s -> %s", __FILE__, \
          __LINE__, #expr, hipGetErrorString (_e));                            \
  } while (0)

#define SCHRO_HIP_REQUIRE(cond, ...)                                           \
  do {                                                                         \
    if (!(cond))                                                               \
      return schro::set_error (SCHRO_HIP_EINVAL, __VA_ARGS__);                 \
  } while (0)

// Every kernel launch of the library goes through SCHRO_LAUNCH.  While a ProfileScope of a
// profiling context is open (schro_hip_profile_enable), the launch carries a start / stop event pair
// (hipExtLaunchKernelGGL): the events take the kernel's own begin and end from the dispatch's completion
// signal -- the duration rocprofv3 reports -- and put nothing else on the queue.  (r02 bracketed every
// launch with two hipEventRecord: 8 us of barrier packets per launch, 0.12 ms per profiled bench step.)
bool profile_launch_events (hipEvent_t * start, hipEvent_t * stop);

#ifdef SCHRO_HIP_DRY
// (the grid and the block are still evaluated: a launch geometry computed from a bad table shows up in UBSAN)
#define SCHRO_LAUNCH(kernel, grid, block, shmem, stream, ...)                                      \
  do {                                                                                             \
    const dim3 g_ = (grid), b_ = (block);                                                          \
    (void) g_; (void) b_; (void) (shmem); (void) (stream);                                         \
  } while (0)
#else
#define SCHRO_LAUNCH(kernel, grid, block, shmem, stream, ...)                                      \
  do {                                                                                             \
    hipEvent_t pa_, pb_;                                                                           \
    if (schro::profile_launch_events (&pa_, &pb_))                                                 \
      hipExtLaunchKernelGGL (kernel, grid, block, shmem, stream, pa_, pb_, 0, __VA_ARGS__);       \
    else                                                                                           \
      hipLaunchKernelGGL (kernel, grid, block, shmem, stream, __VA_ARGS__);                        \
  } while (0)
#endif

// ---- job tables handed to the kernels (device memory, one per launch) ------

// One (plane, level) of the inverse wavelet.
struct IwtJob {
  const void *sb[4];            // LL, HL, LH, HH: element (0,0) of each sub-band
  int sb_stride[4];             // bytes between sub-band rows
  void *dst;
  int dst_stride;
  int w, h;                     // output size of this level (sub-bands are w/2 x h/2)
  int tiles_x;
  int tile_base;                // first block id of this job
  int flags;                    // bit0: all sources 8-byte aligned, bit1: dst 16-byte aligned
  int pad;
  // chain form (iiwt_reg.hip, r04): the job whose output is this job's LL band -- rows of output per tile row
  // (0: none, the coarsest level), its tile grid, its first counter -- this job's own first counter (-1: nobody
  // reads its output in the launch: level 0), and its tile form
  int dep_rows2, dep_tiles_y, dep_tiles_x, dep_ctr;
  int ctr, small;
  // combine form (r04, level 0 of the register kernel): dst is the u8 PICTURE, out_w x out_h inside the
  // iwt-padded w x h; pred: the OBMC prediction to add (u8), NULL: + 128 (a picture without references)
  const uint8_t *pred;
  int pred_stride;
  int out_w, out_h;
  int pad2;
  // level 1 inside level 0 (iiwt_reg.hip, MODE bit 8): this job is level 0 and synthesises its LL band itself from
  // level 1's sub-bands -- LL (level 2's output, or the coefficient frame / the caller's LL plane), HL, LH, HH of the
  // coefficient frame's level-1 view; sb[0] is unused
  const void *l1_sb[4];
  int l1_sb_stride[4];
};

// One (plane, level) of the forward wavelet (iwt_fwd.hip).
struct IwtFwdJob {
  const void *src;              // the level's compact input image: the source plane, or the LL image of the level before
  int src_stride;               // bytes
  int flags;                    // bit0: src takes 8-byte loads, bit1: the bands take 4-sample stores
  void *band[4];                // LL, HL, LH, HH: element (0,0) of each sub-band this level writes
  int band_stride[4];           // bytes between sub-band rows
  int w, h;                     // input size of this level (sub-bands are w/2 x h/2)
  int tiles_x;
  int tile_base;                // first block id of this job
  uint32_t m_tiles_x;           // div_magic (tiles_x)
  int pad;
};

// Where the samples of one component lie in a packed picture's rows or in a planar plane (unpack_fetch.h).
enum { kUnpackU8 = 0, kUnpackS16 = 1, kUnpackS32 = 2, kUnpackV210 = 3, kUnpackU16 = 4 };
struct UnpackSrc {
  const uint8_t *base;          // row 0
  int stride;                   // bytes
  int row_bytes;                // the bytes of a row that exist
  int kind;                     // kUnpack*
  int xmul, xoff;               // sample x is at byte x * xmul + xoff of its row (not v210)
  int comp;                     // v210: the component
  int depth;                    // bytes per sample of the unpacked frame: 1 (u8), 2, 4
};

// One component of one picture of schro_hip_unpack_batch (unpack.hip).  A destination sample (x, y) comes from source
// sample (min (x, xmax) shifted by xsh, min (y, ymax) shifted by ysh): crop / edge extension, then the u8 chroma
// decimation (shift > 0: << 1) or repetition (shift < 0: >> 1).
struct UnpackJob {
  UnpackSrc s;
  uint8_t *dst;
  int dst_stride;
  int w, h;                     // the destination component
  int dst_bpp;
  int xmax, ymax, xsh, ysh;
  int vec;                      // dst and dst_stride are multiples of 16: whole 16-byte pieces
  int tiles_x;
  int tile_base;
};

// Level 0 of the forward wavelet reading a packed picture (iwt_fwd.hip): region sample (x, y) is source sample
// (min (x, xmax), min (y, ymax)) less the format's offset.
struct IwtFwdPackedJob:IwtFwdJob {
  UnpackSrc s;
  int xmax, ymax;
};

// One plane of the downsample (analysis.hip).  A tile is kDownTileCols x kDownTileRows samples of the destination
// INCLUDING its apron: column xorg + 4 * group, row -ext + row.
struct DownsampleJob {
  const uint8_t *src;
  uint8_t *dst;                 // pixel (0, 0)
  int src_stride, dst_stride;
  int sw, sh;                   // source size
  int dw, dh;                   // destination size, (sw + 1) / 2 x (sh + 1) / 2
  int ext;                      // apron samples on every side
  int xorg;                     // column of the first group: -ext, lowered so that the groups' stores are 4-byte aligned
  int tiles_x;
  int tile_base;                // first block id of this job
  uint32_t m_tiles_x;           // div_magic (tiles_x)
  int pad;
};

// One picture of the SAD scan (analysis.hip), and one scan as the kernel reads it
struct ScanPicture {
  const uint8_t *frame;
  const uint8_t *ref;
  SchroHipMetricScanResult *results;
  uint32_t *metrics;            // NULL: no tables
  int frame_stride, ref_stride;
  int width, height;
  int scan_base;                // index of the picture's first scan in the launch
  int pad[3];
};
struct ScanJob {
  int x, y, bw, bh;
  int ref_x, ref_y, sw, sh;
  int gi, gj;                   // the gravity position inside the window
  int dx, dy;                   // the caller's vector
  int pic;
  uint32_t m_sh;                // div_magic (sh)
  int pad[2];
};
static_assert (sizeof (ScanJob) == 64 && sizeof (ScanPicture) == 64, "scan tables: 64-byte records");

// A motion vector record, SchroMotionVector (schromotion.h:20-37): flags (pred_mode, using_global << 2, split << 3),
// metric, chroma_metric, dx[2], dy[2] as int16 -- or, for an intra block, dc[3] in place of dx[] and dy[0]
constexpr int kMvBytes = 20, kMvDwords = kMvBytes / 4;
constexpr int kMvFlags = 0, kMvMetric = 4, kMvChromaMetric = 8, kMvDx = 12, kMvDy = 16;

// One (picture, reference) chain of the rough motion search (rough_hint.hip): the levels the launch runs, coarse to fine,
// each with its planes and its field.  hint NULL: the level scans around the zero vector (the nohint level, every block
// on its own); else the field of the level above -- the level before it in the chain, or the caller's.
struct RoughLevel {
  const uint8_t *frame;
  const uint8_t *ref;
  uint8_t *field;               // x_num_blocks * y_num_blocks SchroMotionVector records, written whole
  const uint8_t *hint;
  int frame_stride, ref_stride;
  int w, h;                     // both planes
  int ext;                      // the apron the frames would have (the kernel clamps coordinates)
  int shift, dist;
  int pad;
};
struct RoughChain {
  int nbx, nby, xb, yb;         // x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma
  int ref;                      // which of dx[], dy[] the chain fills
  int nlevels;
  int pad[2];
  RoughLevel level[SCHRO_HIP_MAX_HIER_LEVELS];
};
static_assert (sizeof (RoughLevel) == 64 && sizeof (RoughChain) == 32 + 64 * SCHRO_HIP_MAX_HIER_LEVELS, "rough search tables");

// One (picture, reference) chain of the hierarchical block matching (hier_bm.hip): the levels the launch runs, coarse to
// fine, each with the three components of its frames and its field.  hint NULL: no parents in the candidate list.
struct HbmLevel {
  const uint8_t *frame[3];
  const uint8_t *ref[3];
  uint8_t *field;               // x_num_blocks * y_num_blocks SchroMotionVector records, written whole
  const uint8_t *hint;
  int frame_stride[3], ref_stride[3];
  int w, h;                     // luma, both frames
  int hs, vs;                   // chroma shifts
  int ext;                      // the apron the frames would have (the kernel clamps coordinates)
  int shift, dist;              // dist: h_range
  int pad[3];
};
struct HbmChain {
  int nbx, nby, xb, yb;         // x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma
  int ref;                      // which of dx[], dy[] the chain fills
  int nlevels;
  int pad[2];
  HbmLevel level[SCHRO_HIP_MAX_HIER_LEVELS + 1];
};
static_assert (sizeof (HbmLevel) == 128 && sizeof (HbmChain) == 32 + 128 * (SCHRO_HIP_MAX_HIER_LEVELS + 1), "block matching tables");

// One (picture, reference) chain of the sub-pel refinement (subpel.hip), as one precision pass sees it.
struct SubpelChain {
  const uint8_t *src;           // the source picture's luma, linear
  const uint8_t *up;            // the reference's tiled upsampled luma
  uint8_t *field;               // the records the pass doubles and refines
  int32_t *table;               // eight errors per block, candidate order
  double lambda;
  int src_stride, up_stride;
  int w, h, ext;
  int nbx, nby, xb, yb;
  int ref;
  int tile_base;                // the chain's first workgroup of the error launch
  int pad;
};
static_assert (sizeof (SubpelChain) == 88, "sub-pel tables");

// One picture of the split-2 mode decision (mode_split2.hip), as both of its launches see it.
struct Split2Job {
  const uint8_t *src[3];        // the source picture: Y, U, V, linear
  const uint8_t *up[2][3];      // the references' tiled upsampled images; pair: [r][1] is the (U, V) pair image
  const uint8_t *field[2];      // the sub-pel field of each reference
  uint8_t *motion;              // the records the level decides
  int32_t *table;               // SCHRO_HIP_SPLIT2_TABLE_INTS per block
  uint8_t *sb;                  // error, entropy, score per superblock
  double lambda;
  int src_stride[3];
  int up_stride[2];             // luma, chroma
  int w, h, cw, ch;
  int ext, nbx, nby, xb, yb;
  int hs, vs, prec, num_refs;
  int pair;
  int tile_base;                // the picture's first workgroup of the metric launch
  int pad;
};
static_assert (sizeof (Split2Job) == 208, "split-2 tables");

// One picture of the whole mode decision (mode_decision.hip): the split-2 level's record, whose table the unchanged
// split2_metric_kernel fills, and what the further levels add.
struct ModeJob {
  Split2Job s;
  const uint8_t *hbm[2][2];     // [reference][0: the level-1 field, 1: the level-2 field] of the block matching
  int32_t *table;               // SCHRO_HIP_MODE_TABLE_INTS per superblock
  uint8_t *trials;              // four SchroHipModeTrial per superblock
  double *stats;                // mc_error, badblock_ratio, dcblock_ratio
  int tile_base;                // the picture's first workgroup of the mode metric launch
  int pad;
};
static_assert (sizeof (ModeJob) == 272, "mode decision tables");

// r05: the three-level s32 Haar transform of a 4:2:2 picture with the v210 copy-out as its epilogue (iiwt_haar.hip)
struct HaarPackJob {
  const void *src[3];           // the coefficient planes (Y, U, V), in-place sub-band layout
  int src_stride[3];
  int w, h;                     // luma transform size = picture size (chroma: w / 2 x h)
  uint8_t *dst;                 // v210 rows: 16 bytes per 6 pixels
  int dst_stride;
  int tiles_x;                  // workgroups per strip of 8 rows
  int tile_base;
};

// The finest level of a 4:2:2 picture's inverse wavelet with the v210 copy-out as its sink (iiwt.hip, iiwt_v210_kernel)
struct V210Job {
  const void *src[3];           // the coefficient planes (Y, U, V), in-place sub-band layout
  int src_stride[3];
  const void *ll[3];            // each component's level-0 LL band: the frame's LL quadrant (depth 1) or a compact plane
  int ll_stride[3];
  int w, h;                     // luma transform size (chroma: w / 2 x h)
  int out_w, out_h;             // the picture inside it
  uint8_t *dst;                 // v210 rows: 16 bytes per 6 pixels; dst and dst_stride 16-byte aligned
  int dst_stride;
  int tiles_x;
  int tile_base;
  int flags;                    // bit c: component c's four bands take 8-byte loads
};

// The finest level of a 4:2:2 / 4:4:4 s16 picture's inverse wavelet with the YUYV / UYVY / AYUV copy-out as its sink (iiwt.hip,
// iiwt_pack8_kernel)
struct Pack8Job {
  const void *src[3];           // the coefficient planes (Y, U, V), in-place sub-band layout
  int src_stride[3];
  const void *ll[3];            // each component's level-0 LL band: the frame's LL quadrant (depth 1) or a compact plane
  int ll_stride[3];
  const uint8_t *pred[3];       // the prediction to add (rows 8-byte aligned, readable up to a multiple of 8 columns);
  int pred_stride[3];           // pred[0] NULL: + 128 (a picture without references)
  int w, h;                     // luma transform size (chroma: w / 2 x h for YUYV / UYVY, w x h for AYUV)
  int out_w, out_h;             // the picture inside it
  uint8_t *dst;                 // packed rows; dst and dst_stride 16-byte aligned
  int dst_stride;
  int tiles_x;
  int tile_base;
  int flags;                    // bit c: component c's four bands take 8-byte loads; bit 3: UYVY byte order
};

// The finest level of a 4:2:2 / 4:4:4 s16 / s32 picture's inverse wavelet with the v216 / ARGB / AY64 copy-out as its sink
// (iiwt.hip, iiwt_wide_kernel)
struct WideJob {
  const void *src[3];           // the coefficient planes (Y, U, V), in-place sub-band layout
  int src_stride[3];
  const void *ll[3];            // each component's level-0 LL band: the frame's LL quadrant (depth 1) or a compact plane
  int ll_stride[3];
  int w, h;                     // luma transform size (chroma: w / 2 x h for v216, w x h for ARGB / AY64)
  int out_w, out_h;             // the picture inside it
  uint8_t *dst;                 // packed rows; dst and dst_stride 16-byte aligned
  int dst_stride;
  int tiles_x;
  int tile_base;
  int flags;                    // bit c: component c's four bands take 8-byte loads; bit 3: AY64 (4:4:4 kernel: else ARGB)
  int shift;                    // schro_frame_shift_right before the convert; 0: none
};

struct ConvertJob {
  const void *src;
  uint8_t *dst;
  int src_stride, dst_stride;
  int w, h;
  int tiles_x;
  int tile_base;
  const uint8_t *pred;          // r04: NULL: + 128 (offsetconvert); else the prediction to add (rrshift6_add's last steps)
  int pred_stride;
  int pad;
};

struct PackJob {
  const uint8_t *src[3];
  uint8_t *dst;
  int src_stride[3];
  int dst_stride;
  int sw, sh;                   // source luma size
  int hs, vs;                   // source chroma shifts
  int w, h;                     // packed picture size
  int format;
  int src_bpp;                  // v210 only: 1, 2 or 4
  int tiles_x;
  int tile_base;
};

struct UpsampleJob {
  const uint8_t *src;
  uint8_t *dst;
  int src_stride, dst_stride;
  int w, h;
  int tiles_x;
  int tile_base;
  // r04: the V plane of a (U, V) pair whose half-pel samples are stored byte-interleaved (see the
  // half-pel layout below); NULL: one plane
  const uint8_t *src_b;
  int src_b_stride;
  int pad;
};

struct ObmcJob {
  const uint8_t *mvs;
  const uint8_t *ref[2];
  const void *residual;
  uint8_t *out;
  int ref_stride[2];
  int residual_stride;
  int out_stride;
  int w, h;
  int nbx, nby;                 // x_num_blocks, y_num_blocks
  int xblen, yblen, xbsep, ybsep, xoff, yoff;   // this component's geometry
  int max_x_blocks, max_y_blocks;       // interior-block limits (schromotion8.c:794-797)
  int mv_shift_x, mv_shift_y;   // chroma MV scaling (0 for luma)
  int prec, wbits, w1, w2;
  int comp;
  int res_bpp;
  int tiles_x;
  int tile_base;
  // item kernel: everything that depends only on the plane's block geometry, worked out
  // on the host (obmc_item_geometry) instead of in every workgroup's prologue; m_* are
  // ceil (2^32 / d) for mdiv ()
  // (ref_ps, ref_cb, r04: how a sample of this component lies in its half-pel planes -- a sample is
  // 1 << ref_ps bytes wide and this component is byte ref_cb of it: 0, 0 one component per image; 1, c the
  // U / V samples of a picture interleaved, see the half-pel layout below.  The struct stays 256 bytes: the
  // kernels keep a copy in scalar registers.)
  int nseg, ref_ps, lpi, ref_cb, ipw, chunk_cap;
  uint32_t m_tiles_x, m_xbsep, m_ybsep, m_nseg, m_lpi;
  uint32_t m_xramp, m_yramp;    // ceil (2^32 / (2 * offset - 1)): get_ramp's division (schromotion.c:40-49)
  int out_s16;                  // r06: `out` is an s16 plane that receives (acc - 8160) >> 6 = the prediction - 128
                                // (orc_rrshift6_s16_ip_2d: schro_motion_render's add = FALSE, schro_motion_render_cuda's dest);
                                // no residual.  r07: the row kernels' residual forms too (obmc_row_body.h: row_finish_s16)
  unsigned long long *stamps;   // scratch runs only (SCHRO_HIP_OBMC_STAMPS): per-workgroup phase stamps
  // row kernel: the second plane of a job.  The U and V planes of a picture have the same
  // blocks, vectors and sample windows, so one workgroup decodes a tile's blocks once and
  // predicts both planes (nplanes == 2); everything not listed here is shared with plane A
  int nplanes;
  int comp_b;
  const uint8_t *ref_b[2];
  const void *residual_b;
  uint8_t *out_b;
  int residual_stride_b, out_stride_b;
};
static_assert (sizeof (ObmcJob) == 256, "ObmcJob: four 64-byte scalar loads");

// One picture's slices (lowdelay.hip).
struct SliceJob {
  const uint8_t *data;
  uint32_t data_bytes;
  int pad;
  void *comp[3];
  int stride[3];
  int pad2;
};

// What every slice of a launch shares (passed by value).
struct SliceParams {
  int depth;
  int iwt_lw, iwt_lh, iwt_cw, iwt_ch;
  int nh, nv;
  int n_bytes, remainder, denom;        // slice_bytes_num / _denom split, schrolowdelay.c:601-602
  int quant_matrix[SCHRO_HIP_LIMIT_SUBBANDS];
  int run_cap;                          // slice_run_kernel: staging words per lane (launch_slices sets it)
};

// One picture of the slice encoder (lowdelay_enc.hip).
struct EncJob {
  const void *comp[3];
  int stride[3];
  int pad;
  uint8_t *out;                 // the slices
  uint8_t *index;               // a base index per slice
  uint32_t *overrun;
  uint32_t *est;                // scratch: per slice and base index 0 .. 64 the high-band bits (luma, chroma)
  int16_t *recon;               // scratch: the reconstructed LL bands, Y then U then V, tight
  int16_t *work;                // scratch: ldenc_choose_kernel's per-thread samples where LDS is too small
};
// ldenc_choose_kernel: where a thread keeps what (in int16 elements; element k of thread t lies at k * threads + t)
struct EncChooseLayout {
  int coef[3];                  // the slice's LL samples per component
  int top[3];                   // the reconstructed row above, from one sample to the left
  int left[3];                  // the reconstructed column to the left
  int row;                      // the row being reconstructed
  int per_thread;
  int threads, lds_bytes, in_lds;
  int recon_off[3];             // the components' LL bands in EncJob::recon
};

struct DcJob {
  void *data;
  int stride;
  int w, h;
  int pad;
};

// One codeblock of the core-syntax dequantisation (dequant.hip).
struct DequantJob {
  void *dst;                    // first sample of the codeblock in the coefficient frame
  const void *src;              // its quantised values (row-major, tight); NULL: zero codeblock
  int dst_stride;
  int w, h;
  int src_bytes;
  uint32_t factor, offset;
  int tiles_x;
  int tile_base;
};

// r04, dequantisation plans: what is fixed per picture geometry (device-resident) ...
struct DequantGeo {
  int dst_offset;               // bytes from the plane's base to the codeblock's first sample
  int dst_stride;
  int w, h;
  int tiles_x;
  int tile_base;
  int plane;                    // index into the run's DequantPlaneDyn table
  int rec;                      // index into the run's SchroHipCodeblock records
};
// ... and per run and plane (the records themselves go up as they are)
struct DequantPlaneDyn {
  void *dst;
  const void *values;
  int is_intra;
  int pad;
};

// One codeblock of the encoder's quantisation (quant.hip): every per-codeblock constant resolved on the host.
enum QuantForm {
  kQuantCopy = 0,               // s16, index 0: quant = coefficient, the coefficient stays
  kQuantShift = 1,              // s16, a multiple of 4: orc_quantdequant2_s16
  kQuantRecip32 = 2,            // s16, index 3: orc_quantdequant3_s16
  kQuantRecip16 = 3,            // s16, the rest: orc_quantdequant1_s16
  kQuantDivide = 4              // s32: schro_quantise_s32
};
struct QuantJob {
  void *coeffs;                 // first sample of the codeblock in the coefficient plane ...
  void *quant;                  // ... and in the quant plane
  SchroHipCodeblockSummary *summary;    // this codeblock's entry
  int stride;                   // bytes between its rows (both planes)
  int w, h;
  int form;
  uint32_t factor;              // schro_table_quant
  uint32_t offset;              // schro_table_offset_1_2 / _3_8: the dead zone, and (+ 2) what dequantisation adds
  int32_t qoff;                 // what is taken from 4 |x|: offset - factor / 2 (quantdequant1 above index 8: one less)
  int shift;                    // (index >> 2) + 2; quantdequant3: + 16
  uint32_t inverse;             // schro_table_inverse_quant
  int tiles_x;
  int tile_base;
  int pad;
};
// The intra LL recurrence: one band per workgroup, the codeblocks that tile it (with their quantisers) behind the jobs.
struct QuantDcJob {
  void *coeffs;
  void *quant;
  SchroHipCodeblockSummary *summary;    // the plane's entries; record k of the band writes entry k
  int stride;
  int w, h;
  int rec_base, nrec;           // its QuantDcRec run
  int pad;
};
struct QuantDcRec {
  int x0, y0, x1, y1;           // samples of the band, x1 / y1 exclusive
  uint32_t factor, offset;
  int index;                    // its summary entry
  int pad;
};
// One sub-band of the histogram launch (hist.hip): its sampled rows as rows x gpr groups of 16 bytes, 2048 per workgroup.
struct HistJob {
  const void *base;             // sample (0, 0) of the band
  uint32_t *counts;             // its SchroHipHistogramCounts: 104 bins, then the overflow word
  int stride;                   // bytes between the band's rows
  int w;
  int skip_shift;               // sampled row r is row r << skip_shift of the band
  int dc;                       // the DC-predict form
  uint32_t gpr;                 // groups per row: div_up (w, 16 / bpp)
  uint32_t items;               // sampled rows x gpr
  uint32_t step_rows, step_groups;      // a lane's step from one of its groups to the next: 256 / gpr, 256 % gpr
  int tile_base;
  int pad;
};

constexpr int kMaxJobs = 256;

// ---- picture statistics (picture_sums.hip, lowpass2.hip, ssim.hip; plane_stats.cpp) ----
struct SumsJob {
  const void *a;
  const uint8_t *b;             // or NULL
  unsigned long long *result;   // two words
  int a_stride, b_stride;
  int w, h, bps;
  int tiles_x;
  int tile_base;
  int pad;
};
struct LowpassJob {
  void *data;
  uint32_t *out_of_range;
  double hc[4], vc[4];
  int stride, w, h, bps;
  int row_base;                 // first workgroup of the row kernel (kLowpassRows rows each)
  int col_base;                 // ... of the column kernel (kLowpassCols columns each)
};
struct SsimJob {
  const uint8_t *a, *b;
  uint8_t *a_low, *b_low;       // scratch, stride8
  int16_t *ab, *aa, *bb;        // scratch, stride16
  double *partial;              // scratch: one double per tile
  SchroHipSsimResult *result;
  double *map;                  // or NULL
  int a_stride, b_stride, stride8, stride16, map_stride;
  int w, h;
  int tiles_x, ntiles;
  int tile_base;
};
// tile geometry of the kernels, for the plane layer's tables and the tests' edge sizes
constexpr int kSumsTileBytes = 1024, kSumsTileRows = 16;
constexpr int kLowpassRows = 64, kLowpassChunk = 128, kLowpassCols = 64, kLowpassColRows = 8;
constexpr int kSsimTileCols = 256, kSsimTileRows = 8;
int launch_plane_sums (hipStream_t stream, const SumsJob * d_jobs, int njobs, int total_tiles);
int launch_lowpass2 (hipStream_t stream, const LowpassJob * d_jobs, int njobs, int row_groups, int col_groups);
int launch_ssim_prepare (hipStream_t stream, const SsimJob * d_jobs, int njobs, int total_tiles);
int launch_ssim_products (hipStream_t stream, const SsimJob * d_jobs, int njobs, int total_tiles);
int launch_ssim_final (hipStream_t stream, const SsimJob * d_jobs, int njobs, int total_tiles);

// XCD-aware workgroup order.  The dispatcher deals workgroups round-robin over
// the 8 XCDs (each with its own 4 MiB L2), so neighbouring tiles -- which share
// lifting halos and reference windows -- would land on 8 different L2s and each
// would fetch its own copy.  This bijection gives every XCD one contiguous run
// of tile ids instead (speed only; any placement is correct).
#ifdef __HIPCC__
// Device pointers reach the kernels inside job structs, so the compiler only knows them
// as generic pointers and would emit flat_load / flat_store: those count on vmcnt AND
// lgkmcnt and return out of order, which forces s_waitcnt 0 before any LDS result is
// used and serialises a software-pipelined load with the work it should overlap.
// gload / gstore say "this is global memory" at the access (global_load / global_store).
// Native vector types only: a class type such as uint2 would be copied through a generic
// reference and fall back to flat.
#define SCHRO_GLOBAL __attribute__ ((address_space (1)))
typedef uint32_t u32x2 __attribute__ ((ext_vector_type (2)));
typedef uint32_t u32x4 __attribute__ ((ext_vector_type (4)));
typedef uint32_t u32_u __attribute__ ((aligned (1)));         // byte-aligned forms
typedef u32x2 u32x2_u __attribute__ ((aligned (1)));
typedef u32x4 u32x4_u __attribute__ ((aligned (1)));

template < typename V, typename P > __device__ __forceinline__ V
gload (const P * p)
{
  return *(const SCHRO_GLOBAL V *) p;
}

template < typename V, typename P > __device__ __forceinline__ void
gstore (P * p, V v)
{
  *(SCHRO_GLOBAL V *) p = v;
}

// the last steps of orc_rrshift6_add_s16_2d / _s32_2d with the prediction p = (acc + 32) >> 6 already there:
// convlw (s32), addw (wraps), convsuswb; p = 128: orc_offsetconvert_u8_s16 / _s32 (a picture without references)
template < typename T >
__device__ __forceinline__ uint8_t
combine_pred (T s, uint32_t p)
{
  const int v = (int16_t) ((int16_t) s + (int16_t) p);
  return (uint8_t) min (max (v, 0), 255);
}

// n / d for 1 <= d <= 1024 and 0 <= n < 2^22 without the ~35-instruction integer division
// sequence (there is no hardware divide): one v_mul_hi_u32 by ceil (2^32 / d).  Tile and
// block geometry (tiles per row, block separation, lanes per item ...) is divided by in
// every workgroup's prologue; the item kernel spent ~500 instructions per wave there.
struct DivMagic {
  uint32_t m[1025];
};
constexpr DivMagic
make_div_magic ()
{
  DivMagic t = { };
  for (uint32_t d = 2; d <= 1024; d++)
    t.m[d] = (uint32_t) ((0x100000000ull + d - 1) / d);
  return t;
}
static __device__ __constant__ DivMagic kDivMagic = make_div_magic ();

__device__ __forceinline__ int
mdiv (int n, int d, uint32_t m)
{
  return d == 1 ? n : (int) __umulhi ((uint32_t) n, m);
}

__device__ __forceinline__ int
fdiv (int n, int d)
{
  if (d > 1024)                 // outside the table (no geometry of this path gets here)
    return n / d;
  return d == 1 ? n : (int) __umulhi ((uint32_t) n, kDivMagic.m[d]);
}

// n / d with the host-side magic m = div_magic (d): no table load in the kernel
__host__ __device__ inline uint32_t
div_magic (int d)
{
  return d <= 1 ? 0u : (uint32_t) ((0x100000000ull + (uint32_t) d - 1) / (uint32_t) d);
}

// Half-pel images (include/schro_hip.h), r03 layout.  The four planes of the reference's upsampled
// frame (integer, h-half, v-half, hv-half: plane = (X & 1) + 2 * (Y & 1) of half-pel sample (X, Y))
// are kept apart, so a block row's prediction samples are CONTIGUOUS bytes of one plane (no
// even / odd split in the kernel) and a tap the block's phase does not use is never fetched.
// A plane row is stored as 32-byte chunks that advance by 16 columns -- every column sits in two
// chunks -- so any run of up to 17 bytes starts inside some chunk and ends inside the same one: a
// lane fetches its row with ONE byte-aligned load, no alignment or phase-select instructions.  One
// 128-byte line = the same chunk of 4 consecutive rows of one plane; the lines of the four planes
// of a (band of 4 rows, chunk) are adjacent (512 bytes), so the other taps of a window are at
// +-128 / +-256 bytes.  kHpApron replicated columns lie in front of column 0 and behind the last
// one -- get_block clamps a block's origin to 32 pixels outside the picture (schromotion8.c:
// 329-330) -- with the reference's sources (schroframe.c:2012-2029: planes 0 and 1 repeat plane
// 0's edge, planes 2 and 3 plane 2's), which is the clamp of the half-pel column to [0, 2w - 2];
// rows are clamped by the kernels.  `stride` = bytes per band of 4 rows = chunks * 512.
//
// r04 -- chroma as (U, V) pairs.  The U and V planes of a 4:2:0 / 4:2:2 picture have the same blocks,
// vectors and sample windows; stored apart, every window was fetched twice (a 6 x 6 chroma window
// touches 2.25 lines per tap and plane).  A PAIR image is the same layout over samples of two bytes
// (U, V): byte column 2 * (column + kHpApron) + c of the plane row, chunks of 32 bytes = 16 byte
// columns of advance = 8 samples, aprons of 2 * kHpApron bytes.  A block row of up to 8 samples plus
// its X + 1 tap is a run of <= 18 bytes that starts at an even byte <= 14 of its chunk: the same one
// load per tap as for a luma row, and it brings both components.  `ps` (sample shift: 0 plane, 1 pair)
// and `cb` (byte of the sample) below select the form; widths in hp_chunks () are SAMPLES.
constexpr int kHpApron = 32;
constexpr int kHpBandRows = 4;

__host__ __device__ __forceinline__ int
hp_chunks (int w, int ps = 0)
{
  return (((w + 2 * kHpApron) << ps) + 15) / 16 + 1;
}

// padded column xp (= plane column + kHpApron) inside its band: chunk xp >> 4, byte xp & 15 (the
// same column is also byte 16 + (xp & 15) of chunk (xp >> 4) - 1)
__host__ __device__ __forceinline__ size_t
hp_col_offset (int xp)
{
  return (size_t) (xp >> 4) * 512 + (size_t) (xp & 15);
}

__host__ __device__ __forceinline__ size_t
hp_row_offset (int y, int stride)
{
  return (size_t) (y >> 2) * (size_t) stride + (size_t) ((y & 3) * 32);
}

// byte offset of half-pel sample (X, Y), 0 <= X <= 2w - 1, 0 <= Y <= 2h - 1 (pair images: of its
// component cb)
__host__ __device__ __forceinline__ size_t
hp_offset (int X, int Y, int stride, int ps = 0, int cb = 0)
{
  return hp_row_offset (Y >> 1, stride) + hp_col_offset ((((X >> 1) + kHpApron) << ps) + cb) + (size_t) (((X & 1) + 2 * (Y & 1)) * 128);
}

__device__ __forceinline__ int
xcd_tile_id (int bid, int nblocks)
{
  constexpr int kXcd = 8;
  const int q = nblocks / kXcd, r = nblocks % kXcd;
  const int x = bid % kXcd, k = bid / kXcd;
  return x * q + (x < r ? x : r) + k;
}

// Which job owns workgroup tile `bid`: the jobs' tile_base values ascend from 0, so the
// answer is (number of jobs with tile_base <= bid) - 1.  The lanes of the wave probe 64
// jobs at a time (one memory round trip instead of a chain of dependent scalar loads,
// which cost ~6.6k cycles per workgroup for the 24 planes of 8 pictures).
template < typename JOB >
__device__ __forceinline__ int
find_job (const JOB * jobs, int njobs, int bid)
{
  const int lane = threadIdx.x & 63;
  int n = 0;
  for (int base = 0; base < njobs; base += 64) {
    const int idx = base + lane;
    const bool le = idx < njobs && gload < int > (&jobs[idx].tile_base) <= bid;
    n += __popcll (__ballot (le));
  }
  return __builtin_amdgcn_readfirstlane (n - 1);
}

// the same for the codeblock launches (dequant.hip, quant.hip), whose job count runs to 2^18: three probes of 64 lanes in the dense arrays of first tiles behind the
// jobs (every 4096th job, every 64th of that run, the 64 of that run)
template < typename JOB >
__device__ __forceinline__ int
find_dequant_job (const JOB * jobs, int njobs, int bid)
{
  const int lane = threadIdx.x & 63;
  const int *first = reinterpret_cast < const int *>(jobs + njobs);
  const int n64 = (njobs + 63) / 64;
  int lo = 0;
  if (njobs > 4096) {
    const int idx = lane;
    const bool le = idx * 4096 < njobs && gload < int > (first + njobs + n64 + idx) <= bid;
    lo = (__popcll (__ballot (le)) - 1) * 4096;
  }
  if (njobs > 64) {
    const int idx = (lo >> 6) + lane;
    const bool le = idx < n64 && gload < int > (first + njobs + idx) <= bid;
    lo += (__popcll (__ballot (le)) - 1) * 64;
  }
  const int idx = lo + lane;
  const bool le = idx < njobs && gload < int > (first + idx) <= bid;
  return __builtin_amdgcn_readfirstlane (lo + __popcll (__ballot (le)) - 1);
}
#endif

// launchers (one per .hip file)
int launch_iiwt_level (hipStream_t stream, const IwtJob * d_jobs, int njobs,
    int total_tiles, int filter, int bpp);

// fused finest levels (iiwt.hip): one launch runs levels nl-1 .. 0
size_t iiwt_fused_job_size (void);
int iiwt_fused_max_levels (int filter, int bpp);
void iiwt_fused_job_fill (void *job, const void *src, int src_stride, int bpp, int nl,
    const void *ll, int ll_stride, void *dst, int dst_stride, int w, int h, int tiles_x,
    int tile_base);
int launch_iiwt_fused (hipStream_t stream, const void *d_jobs, int njobs, int total_tiles,
    int filter, int bpp, int nl);
// element-wise s32 Haar level (iiwt_haar.hip)
bool iiwt_haar_supported (int filter, int bpp);
bool iiwt_haar_job_ok (const IwtJob & j);
void iiwt_haar_geometry (int *cols, int *rows);
int launch_iiwt_haar (hipStream_t stream, const IwtJob * d_jobs, int njobs, int total_tiles, int filter);
// ... all three levels of a depth-3 transform in one pass (r03)
bool iiwt_haar3_job_ok (const void *src, int src_stride, const void *dst, int dst_stride, int w, int h);
void iiwt_haar3_geometry (int *blocks_x, int *blocks_y);
int launch_iiwt_haar3 (hipStream_t stream, const IwtJob * d_jobs, int njobs, int total_tiles, int filter);
// register form of one level (iiwt_reg.hip): s16, filters with a small lifting halo
bool iiwt_reg_supported (int filter, int bpp);
void iiwt_reg_geometry (int filter, int small, int *useful_cols, int *useful_row_pairs,
    int *min_row_pairs);
int launch_iiwt_reg (hipStream_t stream, const IwtJob * d_jobs, int njobs, int total_tiles,
    int filter, int small, int combine, int l1_inline = 0);
// ... level 1 synthesised inside the level-0 tile (large tiles only): the filters built, the tile geometry
bool iiwt_reg_l1_supported (int filter);
void iiwt_reg_l1_geometry (int filter, int *useful_cols, int *useful_row_pairs, int *min_row_pairs);
int launch_iiwt_chain (hipStream_t stream, const IwtJob * d_jobs, const uint32_t * d_order, int n_tiles, uint32_t * ctrl,
    uint32_t run, uint32_t * gave_up, uint32_t epoch, int filter);
void iiwt_tile_geometry (int filter, int bpp, int *useful_cols,
    int *useful_row_pairs);
// one level of the forward wavelet (iwt_fwd.hip)
void iwt_fwd_tile_geometry (int filter, int bpp, int *useful_cols, int *useful_row_pairs);
// ... and the halo of its region: columns per half on either side, row pairs above and below
void iwt_fwd_tile_halo (int filter, int bpp, int *halo_cols, int *halo_row_pairs);
int launch_iwt_fwd_level (hipStream_t stream, const IwtFwdJob * d_jobs, int njobs, int total_tiles, int filter, int bpp);
// ... level 0 with the packed fetch stage (the same tile geometry)
int launch_iwt_fwd_packed (hipStream_t stream, const IwtFwdPackedJob * d_jobs, int njobs, int total_tiles, int filter, int bpp);
// packed picture / planar frame -> planar frame (unpack.hip): a tile is pieces_x 16-byte pieces of `rows` destination rows
void unpack_tile_geometry (int *pieces_x, int *rows);
int launch_unpack (hipStream_t stream, const UnpackJob * d_jobs, int njobs, int total_tiles);
// the downsample and the SAD scan (analysis.hip)
void downsample_tile_geometry (int *cols, int *rows);
int launch_downsample (hipStream_t stream, const DownsampleJob * d_jobs, int njobs, int total_tiles);
// LDS bytes one wave needs for a bw x bh block scanned over sw x sh positions (0: an empty block), and the most a launch gives
size_t scan_lds_bytes (int bw, int bh, int sw, int sh);
size_t scan_lds_limit ();
int launch_metric_scan (hipStream_t stream, const ScanPicture * d_pics, const ScanJob * d_scans, int nscans, size_t lds_per_wave);
// the rough motion search (rough_hint.hip): one workgroup per chain, of as many waves as lds_per_wave allows
int launch_rough_hint (hipStream_t stream, const RoughChain * d_chains, int nchains, size_t lds_per_wave);
// the hierarchical block matching (hier_bm.hip): likewise
int launch_hier_bm (hipStream_t stream, const HbmChain * d_chains, int nchains, size_t lds_per_wave);
// the sub-pel refinement (subpel.hip): the errors of pass mvprec over the blocks of all chains, subpel_error_blocks ()
// blocks per workgroup; and the choice, one workgroup per chain
int subpel_error_blocks ();
int launch_subpel_error (hipStream_t stream, const SubpelChain * d_chains, int nchains, int total_groups, int mvprec);
int launch_subpel_choose (hipStream_t stream, const SubpelChain * d_chains, int nchains, int mvprec);

// the split-2 mode decision (mode_split2.hip): the table entries over the blocks of all pictures, split2_metric_blocks ()
// blocks per workgroup and jobs[].tile_base laid out accordingly; then the choice, one workgroup per picture
int split2_metric_blocks ();
int launch_split2_metric (hipStream_t stream, const Split2Job * d_jobs, int njobs, int total_groups);
int launch_split2_choose (hipStream_t stream, const Split2Job * d_jobs, int njobs);
// the whole mode decision (mode_decision.hip): the table entries of the split-1 / split-0 candidates and the zero-vector
// trial over the superblocks of all pictures, mode_metric_units () waves per superblock and mode_metric_waves () per
// workgroup, jobs[].tile_base laid out accordingly; then the walk, one workgroup per picture
int mode_metric_units ();
int mode_metric_waves ();
int launch_mode_metric (hipStream_t stream, const ModeJob * d_jobs, int njobs, int total_groups);
int launch_mode_choose (hipStream_t stream, const ModeJob * d_jobs, int njobs);
int launch_convert (hipStream_t stream, const ConvertJob * d_jobs, int njobs,
    int total_tiles, int bpp);
void convert_tile_geometry (int *tw, int *th);
int launch_pack (hipStream_t stream, const PackJob * d_jobs, int njobs, int total_tiles);
int launch_shift_right (hipStream_t stream, const ConvertJob * d_jobs, int njobs, int total_tiles, int bpp, int shift);
int launch_add (hipStream_t stream, const ConvertJob * d_jobs, int njobs, int total_tiles, int src_bpp, bool subtract);
void pack_tile_geometry (int *groups_x, int *rows);
// persist_grid > 0 (experiments build): that many persistent workgroups (all jobs of one form: pair images or planes)
int launch_upsample (hipStream_t stream, const UpsampleJob * d_jobs,
    int njobs, int total_tiles, int persist_grid);
void upsample_tile_geometry (int *tw, int *th);
int launch_slices (hipStream_t stream, const SliceJob * d_jobs, int njobs, const SliceParams & P, int bpp, int arith,
    bool aligned16);
bool dc_skew_ok (const DcJob * jobs, int njobs, int bpp);
// edge != NULL: dc_skew_kernel with that hand-over buffer (edge_pitch samples per strip, njobs x strips of
// them, tagged with `epoch`); NULL: dc_predict_kernel
int launch_dc_predict (hipStream_t stream, const DcJob * d_jobs, int njobs, int max_rows, int bpp,
    unsigned long long *edge, int edge_pitch, uint32_t epoch, uint32_t * gave_up);
// the hand-over buffer of the selected queue for a launch of njobs bands of at most max_rows x max_w
int dc_edge_for (SchroHipContext * ctx, int njobs, int max_rows, int max_w, unsigned long long **edge,
    int *edge_pitch, uint32_t * epoch);
// non-zero (the launch's epoch) once a dc_skew_kernel strip or a chain-wavelet tile has given up waiting (a device fault
// of the launch): reported by the next call that looks, enqueueing or synchronising
int dc_gave_up (SchroHipContext * ctx);
// r06: the prediction_only OBMC batches whose predictions did not fit 8 bits -- a per-picture ROUTING answer
// (SCHRO_HIP_ENEEDS_RESIDUAL), looked for by the synchronising calls only (stage completion, schro_hip_synchronize,
// schro_hip_queue_synchronize) and by schro_hip_obmc_overflowed: an unrelated enqueue is never refused for it
int pred_overflow_poll (SchroHipContext * ctx);
// before batch `epoch` is given ring word epoch % kOvfRing: the word's previous owner has finished and its answer is kept
int pred_overflow_claim (SchroHipContext * ctx, uint32_t epoch);
}
// (plane_lowdelay.cpp, beside the plan's other entry points; not part of the public header)
extern "C" bool schro_hip_dequant_plan_matches (const SchroHipDequantPlan * plan, const SchroHipDequantPlane * planes, int nplanes, int bpp, int arith);
namespace schro {
// iiwt_haar.hip, r05
bool iiwt_haar3_v210_ok (const HaarPackJob & j);
int iiwt_haar3_v210_strip_width ();
int launch_iiwt_haar3_v210 (hipStream_t stream, const HaarPackJob * d_jobs, int njobs, int total_tiles, int filter);
// iiwt.hip: the finest level + v210 copy-out of every filter (picture columns / rows per workgroup)
void iiwt_v210_geometry (int filter, int bpp, int *cols, int *rows);
int launch_iiwt_v210 (hipStream_t stream, const V210Job * d_jobs, int njobs, int total_tiles, int filter, int bpp);
// iiwt.hip: the finest level + YUYV / UYVY (ayuv 0) or AYUV (ayuv 1) copy-out of every filter, s16
void iiwt_pack8_geometry (int filter, int ayuv, int *cols, int *rows);
int launch_iiwt_pack8 (hipStream_t stream, const Pack8Job * d_jobs, int njobs, int total_tiles, int filter, int ayuv);
// iiwt.hip: the finest level + v216 (v216 1: columns = output pairs) or ARGB / AY64 (v216 0) copy-out of every filter, s16 / s32
void iiwt_wide_geometry (int filter, int v216, int *cols, int *rows);
int launch_iiwt_wide (hipStream_t stream, const WideJob * d_jobs, int njobs, int total_tiles, int filter, int bpp, int v216);
int launch_dequant (hipStream_t stream, const DequantJob * d_jobs, int njobs, int total_tiles, int bpp, int arith);
int launch_dequant_plan (hipStream_t stream, const DequantGeo * d_geo, int njobs, int total_tiles,
    const SchroHipCodeblock * d_recs, const DequantPlaneDyn * d_planes, int bpp, int arith);
void dequant_tile_geometry (int *tw, int *th);
// quant.hip
void quant_tile_geometry (int *tw, int *th);
void quant_job_constants (QuantJob * job, int quant_index, int is_intra, int bpp);
int launch_quantise (hipStream_t stream, const QuantJob * d_jobs, int njobs, int total_tiles, int bpp);
int launch_quantise_dc (hipStream_t stream, const QuantDcJob * d_jobs, int njobs, const QuantDcRec * d_recs, int max_rows, int bpp);
// schro_hip_quantise_chosen_batch: a run of a call's QuantJobs (or of its QuantDcRecs) that belong to one plane, and the
// plane's row of chosen quant indices on the device; the records' `pad` holds their sub-band.  The resolve launches write
// what quant_job_constants would have (jobs: table entries first .. of the call's jobs; recs: all of the call's)
struct QuantChosen {
  const int32_t *chosen;
  int first, count;
  int is_intra, pad;
};
int launch_quantise_resolve (hipStream_t stream, QuantJob * d_jobs, int njobs, int first, const QuantChosen * d_runs, int nruns, int bpp,
    uint32_t * clamped);
int launch_quantise_resolve_dc (hipStream_t stream, QuantDcRec * d_recs, int nrecs, const QuantChosen * d_runs, int nruns, uint32_t * clamped);
// lowdelay_enc.hip; stages: 1 estimate, 2 choose, 4 pack
int launch_lowdelay_encode (hipStream_t stream, const EncJob * d_jobs, int njobs, const SliceParams & P,
    const EncChooseLayout & L, int stages);
// noarith_enc.hip: one sub-band of one component of one picture.  Its pieces are (band row r, codeblock column x), piece
// r * hc + x; its codeblocks (y, x) in raster order -- schro_hip_codeblock_layout's, by the closed forms xmin = x bw / hc,
// ymin = y bh / vc, which plane_noarith_enc.cpp holds the caller's records against
struct NaSubband {
  const void *base;             // sample (0, 0) of the band in the quant plane
  int stride;                   // bytes between band rows
  int bw, bh, hc, vc;
  int piece_base;               // first of its bh * hc pieces in the call's piece arrays
  int cb_base;                  // first of its hc * vc codeblocks in the call's codeblock arrays
  int row_base;                 // band rows of the picture's sub-bands before it
  int flags;                    // 1: have_zero_flags, 2: have_quant_offset
  int quant_index;              // of codeblock (0, 0)
  int comp, index;
  int pad[2];
};
static_assert (sizeof (NaSubband) == 64, "NaSubband is copied to LDS as 16 words");
struct NaPicture {
  uint8_t *out;
  SchroHipNoarithResult *result;
  uint32_t capacity;            // min (capacity, 2^29): a picture takes less
  int sb_first, nsb;            // its sub-bands in the call's table, stream order
  int cb_first, ncb;            // its codeblocks
  int rows;                     // band rows of all its sub-bands
};
constexpr int kNaMaxSubbands = 3 * SCHRO_HIP_NOARITH_MAX_SUBBANDS;
constexpr int kNaLayoutThreads = 1024;  // the layout workgroup: a picture of more codeblocks is scanned in runs per thread
constexpr int kNaGridX = 1024;  // workgroups per sub-band of the count and pack launches: more pieces are walked in strides
constexpr uint32_t kNaNone = 0xffffffffu;       // a piece or sub-band that is not written
struct NaScratch {              // the selected queue's, per call
  uint32_t *bits, *info, *start;        // per piece: bits of its codes; row sum (16 bits) | non-zero << 16; first bit
  uint32_t *cb_bits, *cb_flags, *cb_pos, *cb_at;        // per codeblock: bits of its values; 1 zero test fails, 2 truly non-zero;
  // payload bits of the picture before it; its first bit in the picture
  uint32_t *sb_at, *sb_len;     // per sub-band: first bit of its header; payload bytes (0: the zero form)
};
// stages: 1 count, 2 layout, 4 clear + pack
int launch_noarith_encode (hipStream_t stream, const NaSubband * d_sbs, int nsbs, const NaPicture * d_pics, int npics,
    const NaScratch & S, int bpp, int grid_x, int clear_x, int stages);
// schro_hip_noarith_encode_chosen_batch: NaSubband::quant_index from d_chosen[picture][comp][index] (device, [3][19])
int launch_noarith_resolve (hipStream_t stream, NaSubband * d_sbs, int nsbs, const int *d_sb_pic, const int32_t * const *d_chosen,
    uint32_t * clamped);
// noarith_dec.hip: the same syntax read back.  One sub-band of one component of one picture, from the host: where its
// samples go and how it is cut into codeblocks (schro_hip_codeblock_layout's closed forms, as above).
struct NdSubband {
  void *coeffs, *quant;         // sample (0, 0) of the band in each plane; quant may be NULL
  int stride;                   // bytes between band rows, both planes
  int bw, bh, hc, vc;
  int cb_base;                  // first of its hc * vc codeblocks in the call's codeblock records
  int pic, comp, index;
  int pad;
};
struct NdPicture {
  const uint8_t *data;
  const uint32_t *bytes_on_device;      // NULL: data_bytes is the length
  SchroHipNoarithDecodeResult *result;
  uint32_t data_bytes;
  int sb_first, nsb;            // its sub-bands in the call's table, stream order
  uint32_t chunk_first, chunk_cap;      // its chunk slots in the call's arrays: data_bytes / 8 + nsb suffice
  int mode, is_intra, compat;
  int pad;
};
// what nd_header_kernel finds in the stream, per sub-band (8 words)
struct NdBand {
  uint32_t first_byte;          // of the payload, from `data`
  uint32_t bytes;               // of the payload, cut at the input's end
  uint32_t length;              // as stated
  uint32_t chunk_base, nchunks; // its chunks among the picture's
  uint32_t quant_index;
  uint32_t flags;               // 1 coded, 2 have_zero_flags, 4 have_quant_offset
  uint32_t pad;
};
constexpr int kNdChunkBits = 64;        // a lane's share of a payload
constexpr int kNdChainThreads = 1024;   // chunks the chain workgroup composes per step
constexpr int kNdLaneThreads = 256;     // workgroup of the chunk-per-lane launches
constexpr int kNdFillGridX = 1024;      // workgroups per sub-band of the fill launch: more row pieces are walked in strides
constexpr int kNdChunkWords = 5, kNdCbWords = 3, kNdBandWords = 8, kNdPicWords = 2;
struct NdScratch {              // the selected queue's, per call
  NdBand *bands;                // per sub-band
  uint32_t *ptotal;             // per picture: chunks in use, spare
  uint32_t *sum;                // per chunk, 2 words: per entry state A, D, F, S 16 bits: completions << 2 | exit state
  uint32_t *rec;                // per chunk, 3 words: codeblock (kNaNone: no code starts here), index of the first code that
                                // starts here, entry state | first bit << 2
  uint32_t *cb;                 // per codeblock, 3 words: first value bit (zero: the flag's bit), quant index | zero << 8, codes that start in the payload
};
// the scratch the call takes, in words (plane_noarith_dec.cpp and its tests)
static inline size_t
nd_scratch_words (size_t chunks, size_t codeblocks, size_t subbands, size_t pictures)
{
  return kNdChunkWords * chunks + kNdCbWords * codeblocks + kNdBandWords * subbands + kNdPicWords * pictures;
}
// stages: 1 header, 2 summary, 4 chain, 8 decode + fill
int launch_noarith_decode (hipStream_t stream, const NdSubband * d_sbs, int nsbs, const NdPicture * d_pics, int npics,
    const NdScratch & S, int bpp, int lane_x, int fill_x, int stages);
// arith_dec.hip: the same headers in front of arithmetic-coded payloads.  The sub-bands are NdSubband records (cb_base is
// not used), a component's 1 + 3 * depth of them one behind the other, so that sub-band index - 3 is the record 3 in front.
struct AdPicture {
  const uint8_t *data;
  const uint32_t *bytes_on_device;      // NULL: data_bytes is the length
  SchroHipArithDecodeResult *result;
  void *coeffs[3], *quant[3];   // the planes, for the clear launch (quant all NULL or none)
  int stride[3], width[3], height[3];
  uint32_t data_bytes;
  int sb_first, nsb;            // its sub-bands in the call's table, stream order
  int mode, is_intra, compat;
};
// a serial chain: the LL band of a component, or the bands of one orientation from the coarsest level to the finest
struct AdTower {
  int sb_first;                 // its first sub-band in the call's table; the next one is 3 further on
  int nbands;
  int pic;
  int pad;
};
// what ad_header_kernel finds in the stream, per sub-band (8 words of queue scratch)
struct AdBand {
  uint32_t first_byte;          // of the payload, from `data`
  uint32_t bytes;               // of the payload, cut at the input's end
  uint32_t length;              // as stated
  uint32_t quant_index;
  uint32_t flags;               // 1 coded, 2 have_zero_flags, 4 have_quant_offset
  uint32_t pad[3];
};
constexpr int kAdBandWords = 8;
constexpr int kAdContexts = 22; // the contexts transform data uses
constexpr int kAdClearGridX = 64;       // workgroups per plane of the clear launch: more rows are walked in strides
// stages: 1 header, 2 clear, 4 decode.  per_lane: a tower per lane instead of per wave (the measured alternative)
int launch_arith_decode (hipStream_t stream, const NdSubband * d_sbs, const AdPicture * d_pics, int npics, const AdTower * d_towers,
    int ntowers, AdBand * bands, int bpp, int stages, int per_lane);
// motion_enc.hip: one picture's motion data.  A superblock owns kMeSbWords words of the call's scratch: what the count
// launch found in it and where the layout launch put it.
struct MePicture {
  const uint8_t *motion;
  uint8_t *out;
  SchroHipMotionEncodeResult *result;
  uint32_t capacity;            // min (capacity, 2^29): a picture takes less
  int nbx, nby;
  int num_refs, have_global;
  int sb_first;                 // its first superblock in the call's scratch
  int pad;
};
constexpr int kMeSections = SCHRO_HIP_MOTION_SECTIONS;
constexpr int kMeLayoutThreads = 256;   // the layout workgroup: a picture of more superblocks is scanned in runs per thread
constexpr int kMeBits = 0, kMeUnits = 9, kMeUnverified = 18, kMeFirst = 19, kMeAsserted = 20, kMePos = 21, kMeSbWords = 32;
// scratch: kMeSbWords words per superblock of the call, then 2 * kMeSections words per picture (each section's header
// bit, its payload's first bit); stages: 1 count, 2 layout, 4 clear, 8 pack
int launch_motion_encode (hipStream_t stream, const MePicture * d_pics, int npics, uint32_t * scratch, int total_sbs, int waves_x, int clear_x,
    int stages);
// motion_dec.hip: the same sections read back.  A picture owns md_picture_words words of the call's scratch, from
// scratch_first on: the sections (kMdSecWords each), per chunk slot the summary (2 words: per entry state A, D, F, S 16
// bits, completions << 2 | exit state) and the entry (2 words: the index of the first code that starts there, the entry
// state), per superblock the split residual, the split and the first unit (the three together padded to an even count),
// per block seven residuals (sections 2 .. 8), the flags and two code indices (ref-1 or DC, ref-2).
struct MdPicture {
  const uint8_t *data;
  const uint32_t *bytes_on_device;      // NULL: data_bytes is the length
  uint8_t *motion;
  SchroHipMotionDecodeResult *result;
  uint64_t scratch_first;
  uint32_t data_bytes, chunk_cap;       // chunk_cap slots: (data_bytes + 7) / 8 + 8 suffice
  int nbx, nby;
  int num_refs, have_global;
};
constexpr int kMdSections = SCHRO_HIP_MOTION_SECTIONS, kMdSecWords = 8;
constexpr int kMdLaneThreads = 256;     // workgroup of the chunk-per-lane launches
constexpr int kMdScanThreads = 256;     // the scan workgroup: a section of more chunks is composed in runs per thread
constexpr int kMdSplitThreads = 64;     // the split walk: a diagonal of superblocks is short (135 at 2160p with 8 x 8 blocks)
constexpr int kMdWalkThreads = 256;     // the mode and value walks
static inline uint32_t
md_chunk_cap (size_t data_bytes)
{
  return (uint32_t) ((data_bytes + 7) / 8 + 8);
}
static inline uint64_t
md_picture_words (size_t data_bytes, uint64_t blocks)
{
  const uint64_t nsb = blocks / 16;
  return (uint64_t) kMdSections * kMdSecWords + 4ull * md_chunk_cap (data_bytes) + ((3 * nsb + 1) & ~1ull) + 10 * blocks;
}
// stages: 1 header, 2 summary, 4 scan, 8 extract, 16 split walk, 32 mode walk, 64 value walk
int launch_motion_decode (hipStream_t stream, const MdPicture * d_pics, int npics, uint32_t * scratch, int lane_x, int stages);
// motion_arith_dec.hip: the same sections behind nine arithmetic coders.  A picture owns ma_picture_words words of the
// call's scratch, from scratch_first on: the sections (kMaSecWords each), per superblock the split residual, the split and
// the first unit (the three together padded to an even count), per block the mode bins of unit n (bit 0 ref-1, bit 1
// ref-2), seven residuals (sections 2 .. 8), the flags and two code indices (ref-1 or DC, ref-2).
struct MaPicture {
  const uint8_t *data;
  const uint32_t *bytes_on_device;      // NULL: data_bytes is the length
  uint8_t *motion;
  SchroHipMotionArithDecodeResult *result;
  uint64_t scratch_first;
  uint32_t data_bytes, pad;
  int nbx, nby;
  int num_refs, have_global;
};
constexpr int kMaSecWords = 4;
static inline uint64_t
ma_picture_words (uint64_t blocks)
{
  const uint64_t nsb = blocks / 16;
  return (uint64_t) kMdSections * kMaSecWords + ((3 * nsb + 1) & ~1ull) + 11 * blocks;
}
// stages: 1 header, 2 split chain, 4 split walk, 8 mode chain, 16 mode walk, 32 value chains, 64 value walk
int launch_motion_arith_decode (hipStream_t stream, const MaPicture * d_pics, int npics, uint32_t * scratch, int stages);
// quant_choose.hip: one picture of the quantiser choice.  Its estimates live in the call's scratch: picture p owns
// 2 * kQcEstimates doubles from p * 2 * kQcEstimates on -- est_entropy [3][19][60], then est_error.
constexpr int kQcBands = SCHRO_HIP_NOARITH_MAX_SUBBANDS, kQcIndices = SCHRO_HIP_QUANT_CHOOSE_INDICES;
constexpr int kQcEstimates = 3 * kQcBands * kQcIndices;
constexpr int kQcTableDoubles = SCHRO_HIP_HISTOGRAM_BINS * kQcIndices;  // one table, stored [104][60]
struct QcPicture {
  const uint32_t *counts[3];    // SchroHipHistogramCounts arrays: 105 words per sub-band
  SchroHipQuantChoice *result;
  double *est_entropy, *est_error;      // the caller's copies, or NULL
  double weight[kQcBands];
  double ratio[3][kQcBands];
  double scale[3];              // sub-band 0, chroma, diagonal
  double target;
  int skip[kQcBands];
  int depth, noarith, engine;
};
// tables: error, then (have_bits) onebits, zerobits, kQcTableDoubles each
int launch_quant_choose (hipStream_t stream, const QcPicture * d_pics, int npics, const double *tables, int have_bits, double *scratch);
// hist.hip
void hist_tile_geometry (int *group_bytes, int *groups_per_tile, int *groups_per_step);
int launch_histogram (hipStream_t stream, const HistJob * d_jobs, int njobs, int total_tiles, int bpp);
int launch_table_copy (hipStream_t stream, void *dst, const void *src, size_t bytes);
// schro_table_quant[i] and schro_table_offset_1_2[i] (intra) / _3_8[i] (inter)
void dequant_tables (int quant_index, int is_intra, uint32_t * factor, uint32_t * offset);
// overflow: NULL, or (prediction_only launches) the word a prediction that does not fit 8 bits is reported in
int launch_obmc (hipStream_t stream, const ObmcJob * d_jobs, int njobs,
    int total_tiles, int prec, int variant, const uint32_t * d_order, uint32_t * overflow);
// The form of a row kernel (obmc_row*.hip) and of a launch that wants one: the reference kind (0 plain planes, 1 half-pel
// images read at half / quarter pel, 3 at eighth pel), nd prediction dwords per block row and segment (2 .. 4), np planes
// per job (1, 2; 3: (U, V) pairs), ns segments per block row (1, 2); nores: a prediction_only launch; weighted: picture
// weights other than 1, 1 / 2.  nd 0: not the row kernels' case (obmc.hip).
struct RowForm {
  int kind, nd, np, ns;
  bool nores, weighted;
  constexpr explicit operator bool () const { return nd != 0; }
  constexpr bool operator== (const RowForm & o) const
  {
    return kind == o.kind && nd == o.nd && np == o.np && ns == o.ns && nores == o.nores && weighted == o.weighted;
  }
};
// row kernels: the form a plane takes as one job (uv: the U plane of a (U, V) job, ref_b the V planes); nores: of a
// prediction_only launch.  False: not their case
RowForm obmc_row_form (const ObmcJob & job, bool uv, bool nores);
bool obmc_row_has_kernel (const RowForm & form);
// obmc_strip.hip (r05): the register-accumulator form for the 12 / 8 block set
bool obmc_strip_ok (const ObmcJob & j);
void obmc_strip_tiles (const ObmcJob & j, int seg_rows, int *strips, int *segs);
int launch_obmc_strip (hipStream_t stream, const ObmcJob * d_jobs, int njobs, int total_items, int seg_rows, bool nores, uint32_t * overflow,
    int cus);
int obmc_row_tile_width (bool uv);
int obmc_row_tile_height ();
int launch_obmc_row (hipStream_t stream, const ObmcJob * d_jobs, int njobs, int total_tiles, const RowForm & form,
    const uint32_t * d_order, uint32_t * overflow, const uint32_t * d_wtabs);
// the weight table of a job's block geometry as the row kernels copy it into LDS (ObmcJob::ipw: its index in d_wtabs)
// words 1 .. 3 of tile (tx, ty)'s record in a row launch's order table (word 0: job << 16 | tile)
void obmc_row_tile_record (const ObmcJob & job, bool uv, int ns, int tx, int ty, uint32_t * rec);
int obmc_row_weight_words (int nd, int ns);
void obmc_row_weight_table (const ObmcJob & job, int nd, int ns, bool uv, uint32_t * out);
// fills the item-kernel geometry fields of a job (obmc.hip)
void obmc_item_geometry (ObmcJob * job);
void obmc_tiles (int variant, int w, int h, int xoff, int *tiles_x, int *tiles_y);

}                               // namespace schro

// ---- the context --------------------------------------------------------------

namespace schro {
struct FrameQuantTable;
struct FrameHistTable;
}

struct SchroHipContext {
  int device;
  SchroHipMemoryDomain *domain; // the SchroMemoryDomain-shaped handle of this context
  // Two in-order queues (HIP streams) per context: the pixel path of one batch of pictures is
  // HBM-bound in the inverse wavelet and issue-bound in OBMC, so a decoder that runs batch k's
  // OBMC on one queue and batch k+1's wavelet + upsample on the other keeps both busy.  Calls
  // go to the selected queue; `stream` is always streams[cur].  Job-table slots, tile-order
  // slots and the wavelet's scratch are per queue, so a launch on one queue never has its
  // tables rewritten by a copy enqueued on the other.
  // r03: four queues -- 0 and 1 for kernels as before, 2 and 3 by convention the host-to-device and
  // the device-to-host copy queue (SCHRO_HIP_QUEUE_H2D / _D2H): copies from / to pinned host memory
  // enqueued there run on the DMA engines beside the kernels of the other queues, ordered by marks.
  static constexpr int kQueues = 4;
  hipStream_t streams[kQueues];
  hipEvent_t queue_ev[kQueues];
  static constexpr int kMarks = 16;
  hipEvent_t marks[kMarks];     // schro_hip_queue_mark / _wait_mark, created on first use
  int cur;
  hipStream_t stream;
  hipEvent_t ev_begin, ev_end;
  bool stage_complete;          // frame-layer stage calls wait for the selected queue before they return (default)

  // size-keyed allocation cache (schrodomain.c:58-137 semantics)
  struct Slot {
    void *ptr;
    size_t size;
    bool in_use;
  };
  std::vector < Slot > slots;
  size_t domain_bytes;

  // Job tables on the device.  A decoder calls the batch entry points with the same few
  // sets of planes over and over (its frame pool), so tables are kept in a small
  // content-addressed cache: a repeated table costs a hash + memcmp on the host and no
  // copy at all; a new one replaces the least recently used slot (one async copy from the
  // slot's pinned mirror, ordered on the stream behind the kernels that still read it).
  struct ArgSlot {
    uint64_t hash;
    size_t bytes;               // 0: empty
    uint64_t last_use;
    hipEvent_t copied;          // the slot's last host -> device copy
    bool copy_pending;
  };
  static constexpr int kArgSlots = 256;        // kArgSlots / kQueues per queue
  static constexpr size_t kArgSlotBytes = 64u << 10;   // >= kMaxJobs OBMC jobs (static_assert in plane_obmc.cpp)
  char *h_args;                 // kArgSlots pinned mirrors
  char *d_args;
  ArgSlot arg_slots[kArgSlots];
  uint64_t arg_clock;

  // optional per-kernel event profiling
  bool profile;
  struct EvPair {
    hipEvent_t a, b;
    int cls;
  };
  std::vector < EvPair > ev_pool;
  size_t ev_used;

  // OBMC tile orders (plane_obmc.cpp obmc_tile_order): device tables of job << 16 | tile, cached by
  // the geometry and references of the launch they were built for
  struct OrderSlot {
    uint64_t hash;
    uint32_t *d;
    uint32_t *h;                // pinned mirror the table is uploaded from
    size_t cap, count;
    uint64_t last_use;
    hipEvent_t copied;          // the slot's last upload
    bool copy_pending;
  };
  static constexpr int kOrderSlots = 16;        // kOrderSlots / kQueues per queue
  OrderSlot order_slots[kOrderSlots];

  // the register wavelet's chain form (plane_iiwt.cpp iiwt_chain): tile orders cached by the batch's geometry, and per
  // queue the ticket + counters its launches synchronise through (left zero by every launch)
  struct ChainSlot {
    uint64_t hash;
    uint32_t *d;
    size_t cap, count;
    uint64_t last_use;
  };
  static constexpr int kChainSlots = 16;        // kChainSlots / kQueues per queue
  ChainSlot chain_slots[kChainSlots];
  uint32_t *chain_ctrl[kQueues];
  size_t chain_ctrl_words[kQueues];
  uint64_t chain_ctrl_hash[kQueues];    // the geometry the counters count for ...
  uint32_t chain_runs[kQueues];         // ... and how many launches of it they have counted

  // grow-only scratch for intermediate LL bands, one per queue
  void *scratch_q[kQueues];
  size_t scratch_size_q[kQueues];
  void *&scratch_ref () { return scratch_q[cur]; }
  // Job tables too large for a table slot (the codeblocks of a whole batch of pictures): four
  // grow-only pinned mirrors + device buffers per queue, used in turn (the host runs up to three
  // batches ahead of the device), never cached (a decoder's codeblock tables differ from picture to
  // picture)
  struct BigTable {
    char *h, *d;
    size_t cap;
    hipEvent_t copied;
    bool pending;
  };
  static constexpr int kBigTables = 4;
  BigTable big_q[kQueues][kBigTables];
  int big_turn[kQueues];
  // dc_skew_kernel's hand-over buffers (one per queue: two launches in flight never share one) and
  // the launch counter their samples are tagged with
  void *dc_edge_q[kQueues];
  size_t dc_edge_size_q[kQueues];
  uint32_t dc_epoch;
  uint32_t *dc_gave_up;         // pinned host words (16): [0] the epoch of a DC launch whose strip gave up, [1] of a chain
                                // wavelet launch, [4 .. 15] r05: a ring of flags, one per prediction_only OBMC batch in turn
  // r05: prediction_only OBMC batches are numbered (1, 2, ...); batch e raises word 4 + e % kOvfRing when one of its
  // predictions does not fit 8 bits, and ovf_epoch[] remembers which batch a ring word was last handed to
  // r05: the frame layer's dequantisation plan (schro_hipframe_dequantise): one geometry at a time
  struct SchroHipDequantPlan *frame_dq_plan;
  void *dq_stage_q[kQueues];    // staging of host-side quantised values, one per queue (in-order reuse)
  size_t dq_stage_size_q[kQueues];
  // r06: the pixel planes of schro_hip_iiwt_pack_v210_batch's two-pass route, one grow-only block per queue (in-order
  // reuse: the next call's transform writes them behind this call's pack on the same queue) -- no allocation, no wait per call
  void *pack_tmp_q[kQueues];
  size_t pack_tmp_size_q[kQueues];
  static constexpr int kOvfRing = 12;
  uint32_t pred_epoch;
  uint32_t ovf_epoch[kOvfRing];         // the batch that owns ring word k (0: nobody)
  hipEvent_t ovf_ev[kOvfRing];          // ... recorded behind its launches (r06): the word is read and handed on only once it has fired
  // r06: batches found raised, oldest first -- not yet named by a synchronising call's status / not yet fetched by
  // schro_hip_obmc_overflowed (nothing is dropped: a word is cleared only into these lists)
  std::vector < uint32_t > ovf_unannounced, ovf_unfetched;
  // r07: planes handed to the OBMC launches of each route (schro_hip_obmc_routes)
  long long obmc_routes[SCHRO_HIP_OBMC_ROUTES] = {};
  // pictures handed to each route of schro_hip_iiwt_pack_v210_batch (schro_hip_v210_routes)
  long long v210_routes[SCHRO_HIP_V210_ROUTES] = {};
  // ... of schro_hip_iiwt_pack_u8_batch (schro_hip_pack8_routes)
  long long pack8_routes[SCHRO_HIP_PACK8_ROUTES] = {};
  // ... of schro_hip_iiwt_pack_wide_batch (schro_hip_wide_routes)
  long long wide_routes[SCHRO_HIP_WIDE_ROUTES] = {};
  // ... of schro_hip_unpack_iwt_batch (schro_hip_unpack_routes)
  long long unpack_routes[SCHRO_HIP_UNPACK_ROUTES] = {};
  int cus;                     // compute units of the device (launch shaping)
  // the frame layer's quantisation table (schro_hipframe_quantise): the codeblock records of one picture geometry and the
  // device summaries behind them
  struct schro::FrameQuantTable *frame_q_table = nullptr;
  // ... and its histogram table (schro_hipframe_subband_histograms): the sub-band records of one picture geometry, the
  // device counts and their pinned host mirror
  struct schro::FrameHistTable *frame_h_table = nullptr;
  // the tables of the quantiser choice (schro_hip_quant_choose_tables): error, onebits, zerobits, transposed
  double *qc_tables = nullptr;
  bool qc_have_bits = false;
  // ... and the device records of its frame-layer call (schro_encoder_choose_quantisers_hip), one per queue
  SchroHipQuantChoice *qc_frame_choice = nullptr;
};

namespace schro {
// returns a device pointer to a copy of [host, host+bytes), valid for launches enqueued
// on the context's stream before the next 63 distinct tables
int push_args (SchroHipContext * ctx, const void *host, size_t bytes,
    void **dev);
// a grow-only device block of one queue (`block`, `size`: the context's members for the selected queue): nothing is
// allocated, freed or waited for while it is large enough; a block that must grow waits for the queue once
int grow_block (SchroHipContext * ctx, void *&block, size_t & size, size_t bytes);
int ensure_scratch (SchroHipContext * ctx, size_t bytes);
// schro_hip_obmc_routes / _v210_routes / _pack8_routes / _wide_routes, each on its array of the context
template < int N > int
read_routes (const char *who, SchroHipContext * ctx, long long (SchroHipContext::*routes)[N], long long *counts, int reset)
{
  SCHRO_HIP_REQUIRE (ctx && counts, "%s: bad arguments", who);
  for (int k = 0; k < N; k++) {
    counts[k] = (ctx->*routes)[k];
    if (reset)
      (ctx->*routes)[k] = 0;
  }
  return 0;
}
// a device copy
// a device copy of a job table of any size, valid for the launches enqueued on the context's stream
// before the fourth call from now on this queue
int push_big_table (SchroHipContext * ctx, const void *host, size_t bytes, void **dev);
// ... built in place: *host is the pinned mirror to fill, big_table_commit sends it
int big_table_begin (SchroHipContext * ctx, size_t bytes, void **host, void **dev);
int big_table_commit (SchroHipContext * ctx, size_t bytes);
// rows of row_bytes bytes, host <-> device or device -> device, enqueued on the selected queue (context.cpp)
int copy_2d_async (SchroHipContext * ctx, void *dst, int dst_stride, const void *src, int src_stride, int row_bytes,
    int height, hipMemcpyKind kind);
// schro_hip_iwt_batch with src == dst allowed (plane_iwt.cpp): the source planes are copied into the queue's scratch
// first, as the frame layer's in-place schro_hipframe_iwt_transform needs
// packed (plane_unpack.cpp): per plane, where level 0 reads a packed picture's rows instead of planes[p].src (which is
// then not looked at)
struct IwtFwdPacked {
  bool packed;
  UnpackSrc s;
  int xmax, ymax;               // the last source sample of the component along each axis: the edge extension's clamp
};
int iwt_batch_run (SchroHipContext * ctx, const SchroHipIwtFwdPlane * planes, int nplanes, int depth, int filter, int bpp,
    bool in_place, const IwtFwdPacked * packed = nullptr);
// the loop of schro_rough_me_heirarchical_scan_nohint over schro_hip_metric_scan_batch (plane_analysis.cpp): fills the
// host SchroMotionVector array and waits for the queue
int rough_scan_nohint_run (SchroHipContext * ctx, const uint8_t * frame, int frame_stride, const uint8_t * ref, int ref_stride,
    int width, int height, int extension, const SchroHipParams * params, int shift, int distance, int ref_index,
    void *motion_vectors);
// the frame layer's rough search on host fields (plane_rough.cpp): the fields go through the queue's scratch, the call
// waits for the queue.  levels[k], fields[k]: level first_shift + k; hint (or NULL): the host field of the level above the
// last one given -- with it every level is a hint level, without it the last level is the nohint level
int rough_me_host_run (SchroHipContext * ctx, const char *who, const SchroHipRoughPlane * levels, int nlevels, int first_shift,
    const SchroHipParams * params, int ref_index, int nohint_distance, int hint_distance, const void *hint, void *const *fields);
// the frame layer's block matching on host fields (plane_hbm.cpp), likewise.  One level (`hint` read, or NULL) when
// h_range > 0: levels[0], fields[0] are level `shift`.  Else the chain: levels[k], fields[k] are level k, k = 0 ..
// nlevels, entry 0 only with_level0
int hbm_host_run (SchroHipContext * ctx, const char *who, const SchroHipHbmPlane * levels, int nlevels, int shift, int h_range,
    int with_level0, const SchroHipParams * params, int ref_index, const void *hint, void *const *fields);
// the frame layer's sub-pel refinement on host fields (plane_subpel.cpp): chains[c].src_field is the HOST field refined in
// place, chains[c].field is not read -- both become scratch of the queue; waits for the queue
int subpel_host_run (SchroHipContext * ctx, SchroHipSubpelChain * chains, int nchains);
// the frame layer's split-2 mode decision (plane_split2.cpp): pic->fields[r] are the HOST fields, pic->motion and
// pic->superblocks are not read -- all become scratch of the queue; `motion` and `superblocks` are the host outputs; waits
// for the queue
int split2_host_run (SchroHipContext * ctx, SchroHipSplit2Picture * pic, void *motion, void *superblocks);
// ---- what the plane layers of the motion stages share (plane_motion.cpp) ----
// the limits: blocks along an axis; a plane of the two searches and its apron; under a tiled upsampled image a block of
// two 16-column loads per row, its apron columns (kHpApron), and a coordinate that fits a vector's 16 bits
constexpr int kMaxMotionBlocks = 1 << 14;
constexpr int kMaxMotionPlaneSize = 1 << 16, kMaxMotionExtension = 1024;
constexpr int kMaxTiledBlock = 32, kMaxTiledExtension = 32, kMaxVector = 32767;
// the refusals of a block grid -- count, size up to max_block, reference index -- in that order; `who` names the call,
// `what` ("picture", "entry", "chain") and c the one refused
int motion_check_blocks (const char *who, const char *what, int c, int nbx, int nby);
int motion_check_block_size (const char *who, const char *what, int c, int xb, int yb, int max_block);
struct MotionGeometry {
  int nbx, nby, xb, yb, ref;
};
int motion_check_geometry (const char *who, const char *what, int c, const MotionGeometry & g, int max_block);
// ... and of a picture whose references are tiled upsampled images: mv_precision; then the picture's size, the extension
// under the block or over the apron, the reach of a coordinate in 16 bits, lambda
int motion_check_precision (const char *who, const char *what, int c, int mv_precision);
int motion_check_picture (const char *who, const char *what, int c, int width, int height, int xb, int yb, int extension, int mv_precision,
    double lambda);
// a range of device memory a call reads or writes, and whose it is (level < 0: the refusal names no level)
struct MotionSpan {
  uintptr_t begin, end;
  bool written;
  int owner, level;
  const char *name;
};
// nothing written overlaps anything else the call reads or writes (a field of another workgroup's, most of all)
int motion_check_spans (const char *who, const char *what, std::vector < MotionSpan > &spans);
// a batch of chains to the device and its launch, with the LDS per wave its largest block and window need
int run_chains (SchroHipContext * ctx, const std::vector < RoughChain > &chains);
int run_chains (SchroHipContext * ctx, const std::vector < HbmChain > &chains);
// plane_split2.cpp, for plane_mode.cpp: the refusals of one picture of the split-2 stage but for the overlaps, its kernel
// record and its spans (`table`: the split-2 table, NULL in a stage call)
int split2_collect (const char *who, const SchroHipSplit2Picture & s, int c, bool stage, void *table, Split2Job & jb, std::vector < MotionSpan > &spans);
// the frame layer's whole mode decision (plane_mode.cpp): pic->fields[r] and pic->hbm_fields[r][] are the HOST fields;
// motion, superblocks, trials (may be NULL) and stats are the host outputs; waits for the queue
int mode_host_run (SchroHipContext * ctx, SchroHipModePicture * pic, void *motion, void *superblocks, void *trials, double *stats);
// v216 / ARGB / AY64 (plane_frameops.cpp)
bool is_wide_format (int format);
// plane_quant.cpp: schro_hip_quantise_batch; allow_empty: records of no width or height are skipped (the frame layer's
// layouts of tiny sub-bands have them), not refused
int quantise_batch_run (SchroHipContext * ctx, const SchroHipQuantPlane * planes, int nplanes, int bpp, bool allow_empty,
    const int32_t * const *chosen = nullptr, uint32_t * clamped = nullptr);
struct FrameQuantTable {
  std::vector < int >key;       // what the records were laid out for
  std::vector < SchroHipCodeblock > recs[3];
  int dc_first[3];              // records of sub-band 0
  size_t total;                 // records of the three components
  // the three components' entries, one after the other: `total` of them PER QUEUE (kQueues runs in one allocation, the
  // selected queue's is used) -- like the scratch and the staging buffers, so that a picture enqueued on one queue never
  // has its summaries cleared or added to by a picture in flight on another
  SchroHipCodeblockSummary *d_summary;
};
void frame_quant_table_free (SchroHipContext * ctx);
// plane_hist.cpp: schro_hip_histogram_batch; allow_empty: bands of no width or height are skipped (their counts stay
// zero), not refused -- the frame layer's tiny sub-bands
int histogram_batch_run (SchroHipContext * ctx, const SchroHipHistogramPlane * planes, int nplanes, int bpp, bool allow_empty);
struct FrameHistTable {
  std::vector < int >key;       // what the bands were laid out for
  std::vector < SchroHipHistogramBand > bands[3];
  size_t total;                 // bands of the three components
  // the three components' counts, one after the other: `total` of them PER QUEUE (kQueues runs in one allocation, the
  // selected queue's is used), on the device and in pinned host memory -- a picture enqueued on one queue never has its
  // counts cleared or added to by a picture in flight on another
  SchroHipHistogramCounts *d_counts, *h_counts;
};
void frame_hist_table_free (SchroHipContext * ctx);
// plane_quant_choose.cpp
void quant_choose_tables_free (SchroHipContext * ctx);
// the launches made while a scope is open are timed under its kernel class (when profiling is on)
struct ProfileScope {
  ProfileScope (SchroHipContext * c, int cls);
  ~ProfileScope ();
};
}
