// encoder_walk.cpp -- the encoder-side host code of the library under the sanitizers, from a stand-alone program: linked
// against the device-free sanitizer objects of the library (make -C schroedinger_amd/csrc dry_asan dry_tsan), compiled
// with the same -fsanitize set, the runtime first by construction -- no preload, no Python in the process.
//
// It carries no case of its own.  tests/encoder_walk_cases.py writes the case file from the modules the device tests
// share: one line per call -- the call's name, the status it must return, integers.  Every "device" buffer (heap in the
// device-free build) is an allocation of its own of exactly the bytes the line says and holds a canary; a call that must
// be refused has to return the line's status, name itself in schro_hip_last_error () and leave every buffer of the call
// as it was.  Public header only.
//
//   encoder_walk asan FILE   the file forwards and backwards in one context (scratch and cached tables growing, then
//                            already large), then once in a fresh context on queue 1
//   encoder_walk tsan FILE   three threads, each with a context on a device of its own, walk the file in three
//                            rotations at once; a fourth drives a scheduler whose pictures make encoder calls
#include "schro_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

namespace {

const unsigned char kCanary = 0xC5;
const size_t kMvBytes = 20;

struct Line {
  int number;
  std::string call;
  int status;
  std::vector < long long >v;
};

struct Failure {
  std::string what;
};

// the integers of a line, in order
struct Reader {
  const Line & line;
  size_t at = 0;
  explicit Reader (const Line & l):line (l) {}
  long long next ()
  {
    if (at >= line.v.size ())
      throw Failure { "the line is too short" };
    return line.v[at++];
  }
  int i () { return (int) next (); }
  size_t z () { return (size_t) next (); }
  void done ()
  {
    if (at != line.v.size ())
      throw Failure { "the line is too long" };
  }
};

// the buffers of one call: exact allocations filled with the canary
struct Buffers {
  SchroHipContext *ctx;
  struct Buf {
    unsigned char *p;
    size_t n;
    bool host;
  };
  std::vector < Buf > bufs;
  std::vector < std::unique_ptr < SchroHipFrame >> frames;
  explicit Buffers (SchroHipContext * c):ctx (c) {}
  ~Buffers ()
  {
    for (Buf & b:bufs)
      if (b.host)
        free (b.p);
      else
        schro_hip_domain_free (ctx, b.p);
  }
  unsigned char *dev (size_t n)
  {
    n = n ? n : 1;
    unsigned char *p = (unsigned char *) schro_hip_domain_alloc (ctx, n);
    if (!p)
      throw Failure { "schro_hip_domain_alloc failed" };
    memset (p, kCanary, n);     // ("device" memory of the device-free build is heap)
    bufs.push_back ({p, n, false});
    return p;
  }
  unsigned char *host (size_t n)
  {
    n = n ? n : 1;
    unsigned char *p = (unsigned char *) malloc (n);
    if (!p)
      throw Failure { "malloc failed" };
    memset (p, kCanary, n);
    bufs.push_back ({p, n, true});
    return p;
  }
  bool untouched () const
  {
    for (const Buf & b:bufs)
      for (size_t k = 0; k < b.n; k++)
        if (b.p[k] != kCanary)
          return false;
    return true;
  }
  // format, width, height, extension, then per component: bytes, offset of pixel (0, 0), stride, width, height
  SchroHipFrame *frame (Reader & r)
  {
    frames.emplace_back (new SchroHipFrame);
    SchroHipFrame *f = frames.back ().get ();
    memset (f, 0, sizeof (*f));
    f->refcount = 1;
    f->domain = schro_hip_context_domain (ctx);
    f->format = r.i ();
    f->width = r.i ();
    f->height = r.i ();
    f->extension = r.i ();
    for (int k = 0; k < 3; k++) {
      SchroHipFrameData & d = f->components[k];
      const size_t bytes = r.z (), off = r.z ();
      d.format = f->format;
      d.data = dev (bytes) + off;
      d.stride = r.i ();
      d.width = r.i ();
      d.height = r.i ();
      d.length = (int) bytes;
      d.h_shift = k ? SCHRO_HIP_FORMAT_H_SHIFT (f->format) : 0;
      d.v_shift = k ? SCHRO_HIP_FORMAT_V_SHIFT (f->format) : 0;
    }
    return f;
  }
};

void
lowdelay_params (Reader & r, SchroHipLowDelayParams * P)
{
  memset (P, 0, sizeof (*P));
  P->transform_depth = r.i ();
  P->iwt_luma_width = r.i ();
  P->iwt_luma_height = r.i ();
  P->iwt_chroma_width = r.i ();
  P->iwt_chroma_height = r.i ();
  P->n_horiz_slices = r.i ();
  P->n_vert_slices = r.i ();
  P->slice_bytes_num = r.i ();
  P->slice_bytes_denom = r.i ();
  for (int k = 0; k < SCHRO_HIP_LIMIT_SUBBANDS; k++)
    P->quant_matrix[k] = r.i ();
}

void
block_params (Reader & r, SchroHipParams * P)
{
  memset (P, 0, sizeof (*P));
  P->x_num_blocks = r.i ();
  P->y_num_blocks = r.i ();
  P->xbsep_luma = r.i ();
  P->ybsep_luma = r.i ();
}

size_t
field_bytes (const SchroHipParams & P)
{
  return (size_t) (P.x_num_blocks > 0 ? P.x_num_blocks : 1) * (size_t) (P.y_num_blocks > 0 ? P.y_num_blocks : 1) * kMvBytes;
}

// ---- one function per call name: builds the arguments from the line, returns the call's status --------------------------

int
do_downsample (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int n = r.i ();
  std::vector < SchroHipDownsamplePlane > pl (n);
  for (auto & p:pl) {
    memset (&p, 0, sizeof (p));
    p.src = b.dev (r.z ());
    p.src_stride = r.i ();
    p.src_width = r.i ();
    p.src_height = r.i ();
    const size_t bytes = r.z (), off = r.z ();
    p.dst = b.dev (bytes) + off;
    p.dst_stride = r.i ();
    p.dst_extension = r.i ();
  }
  return schro_hip_downsample_batch (ctx, pl.data (), n);
}

int
do_metric_scan (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int tables = r.i (), n = r.i ();
  std::vector < SchroHipMetricScanPicture > pics (n);
  std::vector < std::vector < SchroHipMetricScan >> scans (n);
  for (int k = 0; k < n; k++) {
    SchroHipMetricScanPicture & p = pics[k];
    memset (&p, 0, sizeof (p));
    p.width = r.i ();
    p.height = r.i ();
    p.extension = r.i ();
    p.nscans = r.i ();
    p.frame_stride = p.ref_stride = p.width;
    p.frame = b.dev ((size_t) p.width * p.height);
    p.ref = b.dev ((size_t) p.width * p.height);
    scans[k].resize (p.nscans);
    for (auto & s:scans[k]) {
      s.x = r.i (), s.y = r.i (), s.block_width = r.i (), s.block_height = r.i ();
      s.ref_x = r.i (), s.ref_y = r.i (), s.scan_width = r.i (), s.scan_height = r.i ();
      s.gravity_x = r.i (), s.gravity_y = r.i (), s.dx = r.i (), s.dy = r.i ();
    }
    p.scans = scans[k].data ();
    p.results = (SchroHipMetricScanResult *) b.dev ((size_t) p.nscans * sizeof (SchroHipMetricScanResult));
    if (tables)
      p.metrics = (uint32_t *) b.dev ((size_t) p.nscans * SCHRO_HIP_LIMIT_METRIC_SCAN * SCHRO_HIP_LIMIT_METRIC_SCAN * sizeof (uint32_t));
  }
  return schro_hip_metric_scan_batch (ctx, pics.data (), n);
}

int
do_rough_hint (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int n = r.i ();
  std::vector < SchroHipRoughHintPicture > pics (n);
  std::vector < int >hint_alias (n), field_alias (n);
  std::vector < size_t > bytes (n);
  for (int k = 0; k < n; k++) {
    SchroHipRoughHintPicture & p = pics[k];
    memset (&p, 0, sizeof (p));
    const size_t plane = r.z ();
    p.frame = b.dev (plane);
    p.ref = b.dev (plane);
    p.frame_stride = p.ref_stride = r.i ();
    p.width = r.i ();
    p.height = r.i ();
    p.extension = r.i ();
    p.x_num_blocks = r.i ();
    p.y_num_blocks = r.i ();
    p.xbsep_luma = r.i ();
    p.ybsep_luma = r.i ();
    p.shift = r.i ();
    p.distance = r.i ();
    p.ref_index = r.i ();
    bytes[k] = r.z ();
    hint_alias[k] = r.i ();
    field_alias[k] = r.i ();
    p.field = b.dev (bytes[k]);
  }
  // (a picture's own field stands even where it is not handed over: aliases name the fields as allocated)
  std::vector < void *>own (n);
  for (int k = 0; k < n; k++)
    own[k] = pics[k].field;
  for (int k = 0; k < n; k++) {
    pics[k].hint_field = hint_alias[k] >= 0 ? own[hint_alias[k]] : b.dev (bytes[k]);
    if (field_alias[k] >= 0)
      pics[k].field = own[field_alias[k]];
  }
  return schro_hip_rough_hint_batch (ctx, pics.data (), n);
}

int
do_rough_me (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int nohint = r.i (), hint = r.i (), n = r.i ();
  std::vector < SchroHipRoughChain > chains (n);
  std::vector < std::vector < SchroHipRoughPlane >> levels (n);
  for (int c = 0; c < n; c++) {
    SchroHipRoughChain & ch = chains[c];
    memset (&ch, 0, sizeof (ch));
    ch.n_levels = r.i ();
    ch.x_num_blocks = r.i ();
    ch.y_num_blocks = r.i ();
    ch.xbsep_luma = r.i ();
    ch.ybsep_luma = r.i ();
    ch.ref_index = r.i ();
    const size_t bytes = r.z ();
    levels[c].resize (ch.n_levels);
    for (int k = 0; k < ch.n_levels; k++) {
      SchroHipRoughPlane & pl = levels[c][k];
      const size_t plane = r.z (), off = r.z ();
      pl.frame = b.dev (plane) + off;
      pl.ref = b.dev (plane) + off;
      pl.frame_stride = pl.ref_stride = r.i ();
      pl.width = r.i ();
      pl.height = r.i ();
      pl.extension = r.i ();
      if (k < SCHRO_HIP_MAX_HIER_LEVELS)
        ch.fields[k] = b.dev (bytes);
    }
    ch.levels = levels[c].data ();
  }
  return schro_hip_rough_me_batch (ctx, chains.data (), n, nohint, hint);
}

int
do_frame_rough (SchroHipContext *, Reader & r, Buffers & b, bool with_hint)
{
  SchroHipParams P;
  block_params (r, &P);
  const int shift = r.i (), dist = r.i (), ref = r.i ();
  SchroHipFrame *frame = b.frame (r), *ref_frame = b.frame (r);
  void *mvs = b.host (field_bytes (P));
  if (!with_hint)
    return schro_rough_me_heirarchical_scan_nohint_hip (frame, ref_frame, &P, shift, dist, ref, mvs);
  const void *hint = b.host (field_bytes (P));
  return schro_rough_me_heirarchical_scan_hint_hip (frame, ref_frame, &P, shift, dist, ref, hint, mvs);
}

int
do_frame_rough_chain (SchroHipContext *, Reader & r, Buffers & b)
{
  const int n = r.i ();
  SchroHipParams P;
  block_params (r, &P);
  const int ref = r.i ();
  std::vector < SchroHipFrame * >frames (n + 1, nullptr), refs (n + 1, nullptr);
  std::vector < void *>fields (n + 1, nullptr);
  for (int k = 1; k <= n; k++) {
    frames[k] = b.frame (r);
    refs[k] = b.frame (r);
    fields[k] = b.host (field_bytes (P));
  }
  return schro_rough_me_heirarchical_scan_hip (frames.data (), refs.data (), &P, n, ref, fields.data ());
}

int
do_iwt (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int depth = r.i (), filter = r.i (), bpp = r.i (), n = r.i ();
  std::vector < SchroHipIwtFwdPlane > pl (n);
  for (auto & p:pl) {
    memset (&p, 0, sizeof (p));
    p.src = b.dev (r.z ());
    p.src_stride = r.i ();
    p.dst = b.dev (r.z ());
    p.dst_stride = r.i ();
    p.width = r.i ();
    p.height = r.i ();
  }
  return schro_hip_iwt_batch (ctx, pl.data (), n, depth, filter, bpp);
}

int
do_subtract (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int u8 = r.i (), n = r.i ();
  std::vector < SchroHipConvertPlane > pl (n);
  for (auto & p:pl) {
    memset (&p, 0, sizeof (p));
    p.dst = b.dev (r.z ());
    p.dst_stride = r.i ();
    p.src = b.dev (r.z ());
    p.src_stride = r.i ();
    p.width = r.i ();
    p.height = r.i ();
  }
  return schro_hip_subtract_batch (ctx, pl.data (), n, u8);
}

int
do_quantise (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int bps = r.i (), n = r.i ();
  std::vector < SchroHipQuantPlane > pl (n);
  std::vector < std::vector < SchroHipCodeblock >> recs (n);
  for (int k = 0; k < n; k++) {
    SchroHipQuantPlane & p = pl[k];
    memset (&p, 0, sizeof (p));
    p.bytes = r.z ();
    const long long alias = r.next ();
    unsigned char *coeffs = b.dev (p.bytes);
    p.coeffs = coeffs;
    p.quant = alias >= 0 ? coeffs + alias : b.dev (p.bytes);
    p.is_intra = r.i ();
    p.dc_predict_first = r.i ();
    p.dc_width = r.i ();
    p.dc_height = r.i ();
    p.ncodeblocks = r.i ();
    recs[k].resize (r.z ());
    for (auto & c:recs[k]) {
      memset (&c, 0, sizeof (c));
      c.dst_offset = r.i ();
      c.dst_stride = r.i ();
      c.width = r.i ();
      c.height = r.i ();
      c.src_offset = -1;
      c.quant_index = (unsigned char) r.i ();
    }
    p.codeblocks = recs[k].data ();
    p.summary = (SchroHipCodeblockSummary *) b.dev (recs[k].size () * sizeof (SchroHipCodeblockSummary));
  }
  return schro_hip_quantise_batch (ctx, pl.data (), n, bps);
}

int
do_histogram (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int bps = r.i (), n = r.i ();
  std::vector < SchroHipHistogramPlane > pl (n);
  std::vector < std::vector < SchroHipHistogramBand >> bands (n);
  for (int k = 0; k < n; k++) {
    SchroHipHistogramPlane & p = pl[k];
    memset (&p, 0, sizeof (p));
    p.coeffs = b.dev (r.z ());
    p.bytes = r.z ();
    p.nbands = r.i ();
    const int has_counts = r.i ();
    bands[k].resize (r.z ());
    for (auto & d:bands[k]) {
      d.offset = r.i ();
      d.stride = r.i ();
      d.width = r.i ();
      d.height = r.i ();
      d.skip = r.i ();
      d.dc_predict = r.i ();
    }
    p.bands = bands[k].data ();
    if (has_counts)
      p.counts = (SchroHipHistogramCounts *) b.dev (bands[k].size () * sizeof (SchroHipHistogramCounts));
  }
  return schro_hip_histogram_batch (ctx, pl.data (), n, bps);
}

int
do_lowdelay_encode (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int bps = r.i (), n = r.i (), skew = r.i ();
  SchroHipLowDelayParams P;
  lowdelay_params (r, &P);
  const size_t alloc = r.z (), bytes = r.z (), nslices = r.z ();
  std::vector < SchroHipLowDelayEncodePicture > pics (n);
  for (auto & p:pics) {
    memset (&p, 0, sizeof (p));
    for (int k = 0; k < 3; k++) {
      p.comp[k] = b.dev (r.z ());
      p.stride[k] = r.i ();
    }
    p.slices = b.dev (alloc + skew) + skew;
    p.slices_bytes = bytes;
    p.base_index = b.dev (nslices);
    p.overruns = (uint32_t *) b.dev (sizeof (uint32_t));
  }
  return schro_hip_lowdelay_encode_batch (ctx, pics.data (), n, &P, bps);
}

int
do_frame_iwt (SchroHipContext * ctx, Reader & r, Buffers & b)
{
  const int stage = r.i ();
  SchroHipParams P;
  memset (&P, 0, sizeof (P));
  P.transform_depth = r.i ();
  P.wavelet_filter_index = r.i ();
  P.iwt_luma_width = r.i ();
  P.iwt_luma_height = r.i ();
  P.iwt_chroma_width = r.i ();
  P.iwt_chroma_height = r.i ();
  SchroHipFrame *f = b.frame (r);
  schro_hip_context_set_stage_completion (ctx, stage);
  const int rc = schro_hipframe_iwt_transform (ctx, f, &P);
  schro_hip_context_set_stage_completion (ctx, 1);
  return rc;
}

int
do_frame_pair (SchroHipContext *, Reader & r, Buffers & b, int (*call) (SchroHipFrame *, SchroHipFrame *))
{
  SchroHipFrame *dest = b.frame (r), *src = b.frame (r);
  return call (dest, src);
}

void
transform_params (Reader & r, SchroHipParams * P)
{
  memset (P, 0, sizeof (*P));
  P->transform_depth = r.i ();
  P->num_refs = r.i ();
  P->iwt_luma_width = r.i ();
  P->iwt_luma_height = r.i ();
  P->iwt_chroma_width = r.i ();
  P->iwt_chroma_height = r.i ();
}

int
do_frame_quantise (SchroHipContext *, Reader & r, Buffers & b)
{
  SchroHipParams P;
  transform_params (r, &P);
  for (int l = 0; l <= SCHRO_HIP_LIMIT_TRANSFORM_DEPTH; l++)
    P.horiz_codeblocks[l] = r.i ();
  for (int l = 0; l <= SCHRO_HIP_LIMIT_TRANSFORM_DEPTH; l++)
    P.vert_codeblocks[l] = r.i ();
  const int bad_component = r.i (), bad_index = r.i ();
  SchroHipFrame *quant = b.frame (r), *iwt = b.frame (r);
  const int bpp = SCHRO_HIP_FORMAT_DEPTH (iwt->format) == SCHRO_HIP_FORMAT_DEPTH_S32 ? 4 : 2;
  std::vector < int >index[3];
  const int *indices[3];
  SchroHipCodeblockSummary *summary[3];
  for (int k = 0; k < 3; k++) {
    int n = schro_hip_codeblock_layout (k ? P.iwt_chroma_width : P.iwt_luma_width, k ? P.iwt_chroma_height : P.iwt_luma_height,
        P.transform_depth, P.horiz_codeblocks, P.vert_codeblocks, iwt->components[k].stride, bpp, nullptr, 0);
    if (n <= 0)
      n = 1;
    index[k].resize (n);
    for (int c = 0; c < n; c++)
      index[k][c] = (3 * c + k) % 61;
    if (k == bad_component)
      index[k][0] = bad_index;
    indices[k] = index[k].data ();
    summary[k] = (SchroHipCodeblockSummary *) b.host ((size_t) n * sizeof (SchroHipCodeblockSummary));
  }
  return schro_hipframe_quantise (quant, iwt, &P, indices, summary);
}

int
do_frame_histograms (SchroHipContext * ctx, Reader & r, Buffers & b, int base_queue)
{
  SchroHipParams P;
  transform_params (r, &P);
  const int queue = r.i ();
  SchroHipFrame *iwt = b.frame (r);
  const int depth = P.transform_depth >= 0 && P.transform_depth <= 8 ? P.transform_depth : 0;
  const size_t n = (size_t) 3 * (1 + 3 * depth);
  SchroHipHistogram *hists = (SchroHipHistogram *) b.host (n * sizeof (SchroHipHistogram));
  uint32_t *overflow = (uint32_t *) b.host (n * sizeof (uint32_t));
  schro_hip_context_select_queue (ctx, (base_queue + queue) % 2);
  const int rc = schro_hipframe_subband_histograms (iwt, &P, hists, overflow);
  schro_hip_context_select_queue (ctx, base_queue);
  return rc;
}

int
do_frame_lowdelay_encode (SchroHipContext *, Reader & r, Buffers & b)
{
  SchroHipLowDelayParams P;
  lowdelay_params (r, &P);
  const size_t bytes = r.z ();
  SchroHipFrame *iwt = b.frame (r);
  const size_t nslices = P.n_horiz_slices > 0 && P.n_vert_slices > 0 ? (size_t) P.n_horiz_slices * P.n_vert_slices : 1;
  int *overruns = (int *) b.host (sizeof (int));
  return schro_hip_encode_lowdelay_transform_data (iwt, b.host (bytes), bytes, &P, b.host (nslices), overruns);
}

// what a refusal's message must hold: the call names itself (a frame call may be refused by the batch call under it)
struct Name {
  const char *call, *word, *or_word;
};
const Name kNames[] = {
  {"downsample", "downsample_batch", nullptr}, {"metric_scan", "metric_scan_batch", nullptr},
  {"rough_hint", "rough_hint_batch", nullptr}, {"rough_me", "rough_me_batch", nullptr},
  {"frame_rough_nohint", "scan_nohint", nullptr}, {"frame_rough_hint", "scan_hint_hip", "rough_hint_batch"},
  {"frame_rough_chain", "rough_me_heirarchical_scan_hip", "rough_me_batch"}, {"iwt", "iwt_batch", nullptr},
  {"subtract", "subtract_batch", nullptr}, {"quantise", "quantise_batch", nullptr}, {"histogram", "histogram_batch", nullptr},
  {"lowdelay_encode", "lowdelay_encode_batch", nullptr}, {"frame_iwt", "hipframe_iwt_transform", "iwt_batch"},
  {"frame_subtract", "hipframe_subtract", nullptr}, {"frame_add", "hipframe_add", nullptr},
  {"frame_convert", "hipframe_convert", nullptr}, {"frame_quantise", "hipframe_quantise", nullptr},
  {"frame_histograms", "hipframe_subband_histograms", nullptr},
  {"frame_lowdelay_encode", "encode_lowdelay_transform_data", "lowdelay_encode_batch"},
  {"frame_downsample", "hipframe_downsample", nullptr},
};

int
dispatch (SchroHipContext * ctx, const Line & line, Reader & r, Buffers & b, int base_queue)
{
  const std::string & c = line.call;
  if (c == "downsample")
    return do_downsample (ctx, r, b);
  if (c == "metric_scan")
    return do_metric_scan (ctx, r, b);
  if (c == "rough_hint")
    return do_rough_hint (ctx, r, b);
  if (c == "rough_me")
    return do_rough_me (ctx, r, b);
  if (c == "frame_rough_nohint")
    return do_frame_rough (ctx, r, b, false);
  if (c == "frame_rough_hint")
    return do_frame_rough (ctx, r, b, true);
  if (c == "frame_rough_chain")
    return do_frame_rough_chain (ctx, r, b);
  if (c == "iwt")
    return do_iwt (ctx, r, b);
  if (c == "subtract")
    return do_subtract (ctx, r, b);
  if (c == "quantise")
    return do_quantise (ctx, r, b);
  if (c == "histogram")
    return do_histogram (ctx, r, b);
  if (c == "lowdelay_encode")
    return do_lowdelay_encode (ctx, r, b);
  if (c == "frame_iwt")
    return do_frame_iwt (ctx, r, b);
  if (c == "frame_subtract")
    return do_frame_pair (ctx, r, b, schro_hipframe_subtract);
  if (c == "frame_add")
    return do_frame_pair (ctx, r, b, schro_hipframe_add);
  if (c == "frame_convert")
    return do_frame_pair (ctx, r, b, schro_hipframe_convert);
  if (c == "frame_downsample")
    return do_frame_pair (ctx, r, b, schro_hipframe_downsample);
  if (c == "frame_quantise")
    return do_frame_quantise (ctx, r, b);
  if (c == "frame_histograms")
    return do_frame_histograms (ctx, r, b, base_queue);
  if (c == "frame_lowdelay_encode")
    return do_frame_lowdelay_encode (ctx, r, b);
  throw Failure { "no such call" };
}

// one line through the library; false (and a message on stderr) when the call did not do what the line says
bool
run_line (SchroHipContext * ctx, const Line & line, int base_queue)
{
  try {
    Buffers b (ctx);
    Reader r (line);
    const int rc = dispatch (ctx, line, r, b, base_queue);
    r.done ();
    const char *text = schro_hip_last_error ();
    const std::string msg = text ? text : "";
    if (rc != line.status)
      throw Failure { "returned " + std::to_string (rc) + ", the case file says " + std::to_string (line.status) + " (" + msg + ")" };
    if (line.status != SCHRO_HIP_OK) {
      bool named = false;
      for (const Name & n:kNames)
        if (line.call == n.call)
          named = msg.find (n.word) != std::string::npos || (n.or_word && msg.find (n.or_word) != std::string::npos);
      if (!named)
        throw Failure { "the refusal does not name the call: \"" + msg + "\"" };
      if (!b.untouched ())
        throw Failure { "the refused call wrote to a buffer (canary gone): \"" + msg + "\"" };
    } else if (schro_hip_synchronize (ctx) != SCHRO_HIP_OK) {
      throw Failure { std::string ("schro_hip_synchronize: ") + schro_hip_last_error () };
    }
  }
  catch (const Failure & f) {
    fprintf (stderr, "encoder_walk: line %d (%s): %s\n", line.number, line.call.c_str (), f.what.c_str ());
    return false;
  }
  return true;
}

// lines first, first + step ... of the file, `count` of them, wrapping round
bool
walk (SchroHipContext * ctx, const std::vector < Line > &lines, size_t first, long step, size_t count, int base_queue)
{
  const long n = (long) lines.size ();
  long at = (long) first;
  for (size_t k = 0; k < count; k++, at = ((at + step) % n + n) % n)
    if (!run_line (ctx, lines[at], base_queue))
      return false;
  return true;
}

std::vector < Line > read_file (const char *path)
{
  std::vector < Line > lines;
  std::ifstream in (path);
  std::string text;
  int number = 0;
  while (std::getline (in, text)) {
    number++;
    std::istringstream s (text);
    Line l;
    l.number = number;
    if (!(s >> l.call >> l.status))
      continue;
    long long v;
    while (s >> v)
      l.v.push_back (v);
    lines.push_back (l);
  }
  return lines;
}

SchroHipContext *
new_context (int device)
{
  SchroHipContext *ctx = schro_hip_context_new (device);
  if (!ctx) {
    fprintf (stderr, "encoder_walk: schro_hip_context_new (%d): %s\n", device, schro_hip_last_error ());
    exit (2);
  }
  return ctx;
}

int
single_thread (const std::vector < Line > &lines)
{
  const size_t n = lines.size ();
  SchroHipContext *ctx = new_context (0);
  bool ok = walk (ctx, lines, 0, 1, n, 0) && walk (ctx, lines, n - 1, -1, n, 0);
  schro_hip_context_free (ctx);
  if (ok) {
    ctx = new_context (0);
    ok = schro_hip_context_select_queue (ctx, 1) == SCHRO_HIP_OK && walk (ctx, lines, 0, 1, n, 1);
    schro_hip_context_free (ctx);
  }
  return ok ? 0 : 1;
}

struct Picture {
  const std::vector < Line > *lines;
  size_t first, step;
};

// a scheduler picture: every step-th line from `first` on the device's context, on the scheduler's thread
int
picture_func (SchroHipContext * ctx, int, void *priv)
{
  const Picture *p = (const Picture *) priv;
  for (size_t k = p->first; k < p->lines->size (); k += p->step)
    if (!run_line (ctx, (*p->lines)[k], 0))
      return SCHRO_HIP_EINVAL;
  return 0;
}

int
threads (const std::vector < Line > &lines)
{
  const size_t n = lines.size ();
  const int walkers = 3, pictures = 6;
  bool ok[walkers + 1] = { false, false, false, false };
  std::vector < std::thread > pool;
  for (int t = 0; t < walkers; t++)
    pool.emplace_back ([&, t] {
          SchroHipContext *ctx = new_context (t);
          ok[t] = walk (ctx, lines, n * t / walkers, 1, n, 0);
          schro_hip_context_free (ctx);
        }
    );
  pool.emplace_back ([&] {
        const int devices[2] = { 3, 4 };
        SchroHipScheduler *sched = schro_hip_scheduler_new_on (devices, 2);
        if (!sched) {
          fprintf (stderr, "encoder_walk: schro_hip_scheduler_new_on: %s\n", schro_hip_last_error ());
          return;
        }
        std::vector < Picture > work (pictures);
        bool submitted = true;
        for (int k = 0; k < pictures; k++) {
          work[k] = { &lines, (size_t) k, (size_t) 5 * pictures };
          submitted = submitted && schro_hip_scheduler_submit (sched, k, nullptr, 0, 0, picture_func, &work[k], nullptr) >= 0;
        }
        ok[walkers] = schro_hip_scheduler_wait (sched) == 0 && submitted;
        schro_hip_scheduler_free (sched);
      }
  );
  for (auto & t:pool)
    t.join ();
  return ok[0] && ok[1] && ok[2] && ok[3] ? 0 : 1;
}

}                               // namespace

int
main (int argc, char **argv)
{
  if (argc != 3 || (strcmp (argv[1], "asan") && strcmp (argv[1], "tsan"))) {
    fprintf (stderr, "usage: encoder_walk asan|tsan CASEFILE\n");
    return 2;
  }
  const std::vector < Line > lines = read_file (argv[2]);
  if (lines.empty ()) {
    fprintf (stderr, "encoder_walk: %s holds no cases\n", argv[2]);
    return 2;
  }
  const int rc = strcmp (argv[1], "asan") ? threads (lines) : single_thread (lines);
  printf ("encoder_walk %s: %zu lines, %s\n", argv[1], lines.size (), rc ? "FAILED" : "ok");
  return rc;
}
