"""The case file of tests/c/encoder_walk.cpp, the stand-alone driver that walks the encoder-side host code of the library
under the sanitizers (tests/test_encoder_host_sanitized.py writes the file, builds the driver and runs it).

The plane-layer geometries and refusals are not cases of its own: they come from the modules the device tests and the CPU walks already share --
quant_cases, hist_cases, lowdelay_enc_cases, rough_hint_cases, rough_hint_draws, encoder_tail_draws, encoder_front_draws --
and the refusals from the tables those modules keep for the API tests (quant_cases.refusal_table and SUBTRACT_REFUSAL,
hist_cases.refusal_table, rough_hint_cases.REFUSED_MEMBERS, lowdelay_enc_cases.refused_params).  A case added there reaches
the sanitizer run.  The frame-layer lines are this module's own: small frames of every chroma format over the same calls.

One line per call: the call's name, the status it must return, then integers.  Every buffer of a call is described by the
bytes to allocate for it -- exactly what the geometry spans, no slack: the last row ends with its last sample -- so that in
the device-free build, where "device" memory is heap, a host-side copy or clear past a plane is an AddressSanitizer
report.  `build()` returns the lines and, per class of case the walk must hold, how many lines belong to it."""
import collections
import os
import re

import numpy as np

import encoder_front_draws as FD
import encoder_tail_draws as TD
import hist_cases as HC
import hist_ref as H
import lowdelay_enc_cases as LK
import quant_cases as QC
import rough_hint_cases as RK
import rough_hint_draws as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "schro_hip.h")).read()


def define(name):
    return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, HEADER).group(1))


OK, EINVAL, EUNSUPPORTED = define("SCHRO_HIP_OK"), define("SCHRO_HIP_EINVAL"), define("SCHRO_HIP_EUNSUPPORTED")
MAX_BLOCK = define("SCHRO_HIP_LIMIT_BLOCK_SIZE")
MAX_DISTANCE = (define("SCHRO_HIP_LIMIT_METRIC_SCAN") - 1) // 2
MV_BYTES = 20
# the calls the walk must hold, by the name their lines carry
ENTRY_POINTS = ("downsample", "metric_scan", "rough_hint", "rough_me", "frame_rough_nohint", "frame_rough_hint", "frame_rough_chain",
                "iwt", "subtract", "quantise", "histogram", "lowdelay_encode", "frame_iwt", "frame_subtract", "frame_quantise",
                "frame_histograms", "frame_lowdelay_encode", "frame_downsample", "frame_add", "frame_convert")
CLASSES = ("spill", "block_%d_distance_%d" % (MAX_BLOCK, MAX_DISTANCE), "four_levels", "odd_block_counts", "padded_stride", "420", "422",
           "444", "three_unlike_pictures", "three_picture_batch", "iwt_in_place", "iwt_out_of_place", "scan_tables_on", "scan_tables_off", "subtract_s16",
           "subtract_u8") + tuple("iwt_filter_%d" % f for f in range(7)) + tuple("iwt_depth_%d" % d for d in (1, 2, 3, 4))
FORMATS = {420: (1, 1), 422: (1, 0), 444: (0, 0)}
DEPTH_BITS = {1: 0x00, 2: 0x04, 4: 0x08}


def span(rows, row_bytes, stride):
    """bytes from a plane's first sample to the end of its last row"""
    return max((rows - 1) * stride + row_bytes, 1)


class Walk:
    def __init__(self):
        self.lines, self.classes = [], collections.Counter()

    def add(self, call, status, ints, classes=()):
        assert call in ENTRY_POINTS, call
        self.lines.append("%s %d %s" % (call, status, " ".join(str(int(v)) for v in ints)))
        self.classes.update(set(classes))
        if status != OK:
            self.classes["status_%d" % status] += 1
            self.classes["refused_" + call] += 1


def frame(bpp, hs, vs, w, h, pad=0, ext=0):
    """A planar device frame of three exact allocations: format, width, height, extension, then per component the bytes
    to allocate, the offset of pixel (0, 0), the stride and the size.  Chroma sizes round up, as schro_frame_new does."""
    out = [DEPTH_BITS[bpp] | hs | 2 * vs, w, h, ext]
    for k in range(3):
        cw, ch = (w, h) if k == 0 else (-(-w // (1 << hs)), -(-h // (1 << vs)))
        stride = (cw + 2 * ext) * bpp + pad
        out += [span(ch + 2 * ext, (cw + 2 * ext) * bpp, stride), ext * stride + ext * bpp, stride, cw, ch]
    return out


def lowdelay_ints(P):
    return [P[k] for k in ("transform_depth", "iwt_luma_width", "iwt_luma_height", "iwt_chroma_width", "iwt_chroma_height",
                           "n_horiz_slices", "n_vert_slices", "slice_bytes_num", "slice_bytes_denom")] + list(P["quant_matrix"])[:19]


def shifts_of(P):
    return int(P["iwt_chroma_width"] < P["iwt_luma_width"]), int(P["iwt_chroma_height"] < P["iwt_luma_height"])


def format_of(P):
    """(where rounding to the transform's size has made luma and chroma alike the sizes do not tell: None)"""
    return {v: k for k, v in FORMATS.items()}.get(shifts_of(P))


# ---- the analysis front end ---------------------------------------------------------------------------------------------

def analysis(walk, rounds):
    for down, pictures, tables in FD.analysis_batches(rounds):
        ints = [len(down)]
        for d in down:
            dw, dh = (d["w"] + 1) // 2 + 2 * d["ext"], (d["h"] + 1) // 2 + 2 * d["ext"]
            ints += [span(d["h"], d["w"], d["src_stride"]), d["src_stride"], d["w"], d["h"], span(dh, dw, d["dst_stride"]),
                     d["ext"] * d["dst_stride"] + d["ext"], d["dst_stride"], d["ext"]]
        walk.add("downsample", OK, ints, ["padded_stride"] if any(d["src_stride"] > d["w"] for d in down) else [])
        ints = [int(tables), len(pictures)]
        for p in pictures:
            ints += [p["w"], p["h"], p["ext"], len(p["scans"])] + [int(v) for s in p["scans"] for v in s.tolist()]
        walk.add("metric_scan", OK, ints, ["scan_tables_on" if tables else "scan_tables_off"])
    # the frame layer: a pyramid level of every chroma format, the destination with and without an apron
    for (w, h, fmt, ext) in ((176, 144, 420, 32), (175, 143, 422, 8), (33, 17, 444, 0)):
        hs, vs = FORMATS[fmt]
        cw, ch = -(-w // (1 << hs)), -(-h // (1 << vs))
        # (the destination's chroma is half of the SOURCE's chroma, rounded up: built component by component)
        dest = [DEPTH_BITS[1] | hs | 2 * vs, (w + 1) // 2, (h + 1) // 2, ext]
        for (a, b) in ((w, h), (cw, ch), (cw, ch)):
            dw, dh = (a + 1) // 2, (b + 1) // 2
            stride = dw + 2 * ext + 3
            dest += [span(dh + 2 * ext, dw + 2 * ext, stride), ext * stride + ext, stride, dw, dh]
        walk.add("frame_downsample", OK, dest + frame(1, hs, vs, w, h), [str(fmt)])
    walk.add("frame_downsample", EINVAL, frame(1, 1, 1, 64, 48) + frame(1, 1, 1, 64, 48))          # not half the source


def rough(walk, draws):
    def picture(c, stride=None):
        n = max(c["nbx"], 1) * max(c["nby"], 1) * MV_BYTES
        stride = c["w"] + c["pad"] if stride is None else stride
        return [span(c["h"], c["w"], max(stride, c["w"])), stride, c["w"], c["h"], c["ext"], c["nbx"], c["nby"], c["xb"], c["yb"],
                c["shift"], c["dist"], c["ref_index"], n]

    def classes(pics):
        out = []
        for c in pics:
            if c["xb"] == c["yb"] == MAX_BLOCK and c["dist"] == MAX_DISTANCE:
                out.append("block_%d_distance_%d" % (MAX_BLOCK, MAX_DISTANCE))
            if c["nbx"] % 2 and c["nby"] % 2 and c["nbx"] > 1 and c["nby"] > 1:
                out.append("odd_block_counts")
            if c["pad"]:
                out.append("padded_stride")
        if len(pics) >= 3 and len({(c["w"], c["h"], c["shift"], c["xb"]) for c in pics}) == len(pics):
            out.append("three_unlike_pictures")
        return out

    def hint_line(pics, status=OK, aliases=None, strides=None):
        ints = [len(pics)]
        for k, c in enumerate(pics):
            hint_alias, field_alias = (aliases or {}).get(k, (-1, -1))
            ints += picture(c, (strides or {}).get(k)) + [hint_alias, field_alias]
        walk.add("rough_hint", status, ints, classes(pics))

    for name in sorted(RK.CASES):
        hint_line([RK.CASES[name]])
    # tests/test_gpu_rough_hint.py::test_three_unlike_pictures_in_one_call
    hint_line([RK.CASES[n] for n in ("ref_1_shift2", "block_16x8", "shift3_odd")])
    for n in range(0, RD.N_DRAWS, draws):
        hint_line([{k: v for k, v in c.items() if k not in ("frame", "ref", "hint")} for c in RD.draw(n)])
    # test_a_refused_call_writes_nothing: the second of two pictures spoilt, one member at a time, then the aliasings
    good = RK.CASES[RK.REFUSED_CASE]
    for member, value in RK.REFUSED_MEMBERS:
        if member == "stride":
            hint_line([good, good], EINVAL, strides={1: good["w"] + good["pad"] + value})
        else:
            hint_line([good, dict(good, **{member: value})], EINVAL)
    assert RK.REFUSED_ALIASES == ("hint_is_own_field", "field_is_first_field")
    hint_line([good, good], EINVAL, aliases={1: (1, -1)})
    hint_line([good, good], EINVAL, aliases={1: (-1, 0)})

    # the chain on the plane layer and the three frame calls: tests/test_gpu_rough_hint.py's sizes and level counts, both
    # references of a picture as two chains of one call
    for (w, h) in ((128, 96), (101, 75)):
        for n_levels in (1, 2, 3, 4):
            ext = 32 if n_levels == 3 else 0
            nbx, nby = -(-w // 8), -(-h // 8)
            levels, lw, lh = [], w, h
            for _ in range(n_levels):
                lw, lh = (lw + 1) // 2, (lh + 1) // 2
                levels.append((lw, lh))
            ints = [12, 4, 2]
            for ref in (0, 1):
                ints += [n_levels, nbx, nby, 8, 8, ref, nbx * nby * MV_BYTES]
                for (a, b) in levels:
                    stride = a + 2 * ext
                    ints += [span(b + 2 * ext, stride, stride), ext * stride + ext, stride, a, b, ext]
            walk.add("rough_me", OK, ints, ["four_levels"] if n_levels == 4 else [])
            fr = []
            for (a, b) in levels:
                fr += frame(1, 0, 0, a, b, 0, ext) + frame(1, 0, 0, a, b, 0, ext)
            walk.add("frame_rough_chain", OK, [n_levels, nbx, nby, 8, 8, 0] + fr, ["four_levels"] if n_levels == 4 else [])
    walk.add("rough_me", EINVAL, [MAX_DISTANCE + 1, 4, 1, 1, 8, 6, 8, 8, 0, 8 * 6 * MV_BYTES, span(24, 32, 32), 0, 32, 32, 24, 0])
    walk.add("frame_rough_chain", EINVAL, [1, 0, 6, 8, 8, 0] + frame(1, 0, 0, 32, 24) + frame(1, 0, 0, 32, 24))      # no blocks
    for name in ("partial_blocks", "ref_1_shift2", "beyond_the_picture"):       # test_frame_layer_hint_level
        c = RK.CASES[name]
        two = frame(1, 0, 0, c["w"], c["h"], 0, c["ext"]) + frame(1, 0, 0, c["w"], c["h"], 0, c["ext"])
        walk.add("frame_rough_hint", OK, [c["nbx"], c["nby"], c["xb"], c["yb"], c["shift"], c["dist"], c["ref_index"]] + two)
        walk.add("frame_rough_nohint", OK, [c["nbx"], c["nby"], c["xb"], c["yb"], c["shift"], 12, c["ref_index"]] + two)
    c = RK.CASES["partial_blocks"]
    two = frame(1, 0, 0, c["w"], c["h"]) + frame(1, 0, 0, c["w"], c["h"])
    walk.add("frame_rough_hint", EINVAL, [c["nbx"], c["nby"], c["xb"], c["yb"], c["shift"], MAX_DISTANCE + 1, 0] + two)
    walk.add("frame_rough_nohint", EINVAL, [c["nbx"], c["nby"], c["xb"], c["yb"], c["shift"], 0, 0] + two)


# ---- the forward wavelet, the residual -----------------------------------------------------------------------------------

def forward(walk, rounds):
    for depth, filt, dtype, planes in FD.forward_batches(rounds):
        b = np.dtype(dtype).itemsize
        ints = [depth, filt, b, len(planes)]
        for (w, h, ss, ds) in planes:
            ints += [span(h, w * b, ss), ss, span(h, w * b, ds), ds, w, h]
        walk.add("iwt", OK, ints, ["iwt_out_of_place", "iwt_filter_%d" % filt, "iwt_depth_%d" % depth])
    # every filter at every depth 1 .. 4, out of place and (the frame layer) in place, every chroma format, iwt padding:
    # a 50 x 38 picture in a transform rounded up to a multiple of 1 << depth
    n = 0
    for filt in TD.FILTERS:
        for depth in (1, 2, 3, 4):
            fmt = TD.FORMATS[n % 3]
            b = (2, 4)[n % 2]
            n += 1
            P = LK.params(50, 38, fmt, depth, 1, 1, 1)
            hs, vs = FORMATS[fmt]
            sizes = [(P["iwt_luma_width"], P["iwt_luma_height"])] + [(P["iwt_chroma_width"], P["iwt_chroma_height"])] * 2
            ints = [depth, filt, b, 3]
            for (w, h) in sizes:
                ints += [span(h, w * b, w * b), w * b, span(h, w * b, w * b + 6 * b), w * b + 6 * b, w, h]
            walk.add("iwt", OK, ints, ["iwt_out_of_place", "iwt_filter_%d" % filt, "iwt_depth_%d" % depth, "padded_stride"])
            fw, fh = max(sizes[0][0], sizes[1][0] << hs), max(sizes[0][1], sizes[1][1] << vs)
            walk.add("frame_iwt", OK, [n % 2, depth, filt] + [v for s in sizes[:2] for v in s] + frame(b, hs, vs, fw, fh, 2 * b),
                     ["iwt_in_place", "iwt_filter_%d" % filt, "iwt_depth_%d" % depth, str(fmt)])
    # refusals: a transform larger than the frame; a size that is no multiple of 1 << depth; a u8 frame
    walk.add("frame_iwt", EINVAL, [1, 3, 2, 328, 240, 160, 120] + frame(2, 1, 1, 320, 240))
    walk.add("frame_iwt", EINVAL, [1, 5, 2, 320, 240, 160, 120] + frame(2, 1, 1, 320, 240))
    walk.add("frame_iwt", EINVAL, [1, 2, 0, 320, 240, 160, 120] + frame(1, 1, 1, 320, 240))
    walk.add("iwt", EINVAL, [2, 0, 2, 1, span(64, 124, 128), 128, span(64, 124, 128), 128, 62, 64])
    walk.add("iwt", EINVAL, [2, 7, 2, 1, span(64, 128, 128), 128, span(64, 128, 128), 128, 64, 64])


def residual(walk):
    """schro_hip_subtract_batch and schro_hipframe_subtract / _add / _convert as the encoder loop uses them
    (tests/encode_loop_draws.py): picture - prediction into the iwt-padded s16 frame, reconstruction + prediction,
    the reconstruction to u8; the three chroma formats, odd sizes."""
    for n, (w, h, fmt) in enumerate(((50, 38, 420), (45, 35, 422), (33, 17, 444))):
        hs, vs = FORMATS[fmt]
        P = LK.params(w, h, fmt, 3, 1, 1, 1)
        fw, fh = max(P["iwt_luma_width"], P["iwt_chroma_width"] << hs), max(P["iwt_luma_height"], P["iwt_chroma_height"] << vs)
        for u8 in (1, 0):
            b = 1 if u8 else 2
            ints = [u8, 3]
            for k in range(3):
                cw, ch = (w, h) if k == 0 else (-(-w // (1 << hs)), -(-h // (1 << vs)))
                ds, ss = 2 * cw + 2 * (n + 1), b * cw + b * n
                ints += [span(ch, 2 * cw, ds), ds, span(ch, b * cw, ss), ss, cw, ch]
            walk.add("subtract", OK, ints, ["subtract_u8" if u8 else "subtract_s16", "padded_stride", str(fmt)])
            walk.add("frame_subtract", OK, frame(2, hs, vs, fw, fh, 2) + frame(b, hs, vs, w, h, b * n), [str(fmt)])
            walk.add("frame_add", OK, frame(2, hs, vs, fw, fh, 2) + frame(b, hs, vs, w, h, b * n), [str(fmt)])
        walk.add("frame_convert", OK, frame(1, hs, vs, w, h, 3) + frame(2, hs, vs, fw, fh, 2), [str(fmt)])
        walk.add("frame_convert", OK, frame(1, hs, vs, w, h, 3) + frame(1, hs, vs, w, h), [str(fmt)])
    # quant_cases.SUBTRACT_REFUSAL (a destination stride shorter than its row, over the refusal planes); unlike formats;
    # u8 -> s16
    rows, width = QC.REFUSAL_PLANE
    ds, sw, sh = QC.SUBTRACT_REFUSAL
    walk.add("subtract", EINVAL, [0, 1, span(rows, 2 * width, 2 * width), ds, span(rows, 2 * width, 2 * width), 2 * width, sw, sh])
    walk.add("frame_subtract", EINVAL, frame(2, 1, 1, 64, 48) + frame(4, 1, 1, 64, 48))
    walk.add("frame_add", EINVAL, frame(2, 1, 1, 64, 48) + frame(2, 1, 0, 64, 48))
    walk.add("frame_convert", EUNSUPPORTED, frame(2, 1, 1, 64, 48) + frame(1, 1, 1, 64, 48))


# ---- the quantiser, the histograms ----------------------------------------------------------------------------------------

def quant_plane(spec, quant_alias=-1, ncodeblocks=None, dc=None):
    buf = spec["buf"]
    dc = spec.get("dc") if dc is None else dc
    recs = spec["records"]
    out = [buf.shape[0] * buf.shape[1] * buf.dtype.itemsize, quant_alias, spec["intra"]] + list(dc or (0, 0, 0))
    out += [len(recs) if ncodeblocks is None else ncodeblocks, len(recs)]
    for r in recs:
        out += r[:5]
    return out


def quantise(walk, every):
    def call(specs):
        b = specs[0]["buf"].dtype.itemsize
        ints = [b, len(specs)]
        for s in specs:
            ints += quant_plane(s)
        walk.add("quantise", OK, ints, ["three_unlike_pictures"] if len({s["buf"].shape for s in specs}) >= 3 else [])

    for dtype, seed in ((np.int16, 1), (np.int32, 2)):
        call(QC.geometry_specs(dtype, seed))
        call(QC.dc_specs(dtype, seed, define("SCHRO_HIP_QUANTISE_DC_THREADS")))
    for n, draw in enumerate(TD.quantise_draws()):
        if n % every == 0:
            call(draw["specs"])
    # quant_cases.refusal_table: the bad plane is the second of the call, behind a good one
    rows, width = QC.REFUSAL_PLANE
    stride = 2 * width
    good, cases = QC.refusal_table(stride)
    plane = lambda records: dict(buf=np.zeros((rows, width), np.int16), records=records, intra=0)
    for name, (kw, words) in cases.items():
        kw = dict(kw)
        bad = plane(kw.pop("records"))
        bps = kw.pop("bps", 2)
        dc = (kw.pop("dc_predict_first"), kw.pop("dc_width"), kw.pop("dc_height")) if "dc_predict_first" in kw else None
        ints = [bps, 2] + quant_plane(plane(good)) + quant_plane(bad, kw.pop("quant_offset", -1), kw.pop("ncodeblocks", None), dc)
        assert not kw, (name, kw)
        walk.add("quantise", EINVAL, ints)
    # the frame layer (tests/dry_run_quant_cases.py's geometries over the three chroma formats; 16 x 16 at depth 3 has
    # empty codeblocks: a 1 x 1 chroma LL) and its refusals: a quant index out of range, frames of unlike depth
    n = 0
    for (b, w, h, depth, hc, vc, intra) in ((2, 64, 48, 2, [1, 2, 3], [1, 2, 2], 1), (4, 64, 48, 2, [2, 1, 4], [1, 1, 3], 0),
                                           (2, 16, 16, 3, [2, 2, 2, 2], [2, 2, 2, 2], 1), (2, 64, 48, 2, [1, 2, 3], [1, 2, 2], 0)):
        for fmt in TD.FORMATS:
            hs, vs = FORMATS[fmt]
            head = [depth, 0 if intra else 1, w, h, w >> hs, h >> vs] + (hc + [1] * 7)[:7] + (vc + [1] * 7)[:7]
            two = frame(b, hs, vs, w, h, 2 * b * (n % 3)) + frame(b, hs, vs, w, h, 2 * b * (n % 3))
            walk.add("frame_quantise", OK, head + [-1, 0] + two, [str(fmt)])
            n += 1
        walk.add("frame_quantise", EINVAL, head + [1, 61] + two)
        walk.add("frame_quantise", EINVAL, head + [-1, 0] + frame(6 - b, hs, vs, w, h) + frame(b, hs, vs, w, h))


def histogram(walk, every):
    def call(specs):
        b = specs[0]["buf"].dtype.itemsize
        ints = [b, len(specs)]
        for s in specs:
            nbytes = s["buf"].shape[0] * s["buf"].shape[1] * b
            ints += [nbytes, nbytes, len(s["bands"]), 1, len(s["bands"])] + [v for bd in s["bands"] for v in bd]
        walk.add("histogram", OK, ints, ["three_unlike_pictures"] if len({s["buf"].shape for s in specs}) >= 3 else [])

    for dtype, seed in ((np.int16, 3), (np.int32, 4)):
        call(HC.mixed_specs(dtype, seed))
    for n, draw in enumerate(TD.histogram_draws()):
        if n % every == 0:
            call(draw["specs"])
    # hist_cases.refusal_table: the bad plane is the second of the call, behind a good one
    rows, width = HC.REFUSAL_PLANE
    nbytes = rows * 2 * width
    good, cases = HC.refusal_table(2 * width)
    for name, (kw, words) in cases.items():
        kw = dict(kw)
        bad = kw.pop("bands")
        ints = [kw.pop("bps", 2), 2, nbytes, nbytes, len(good), 1, len(good)] + [v for bd in good for v in bd]
        # (allocated: the plane; claimed: what the case says; bands the call is told of; counts or none; bands in the table)
        ints += [nbytes, kw.pop("bytes", nbytes), kw.pop("nbands", len(bad)), int(kw.pop("counts", 1) is not None), len(bad)]
        ints += [v for bd in bad for v in bd]
        assert not kw, (name, kw)
        walk.add("histogram", EINVAL, ints)
    # the frame layer (tests/dry_run_hist_cases.py's geometries), on both queues
    for (b, w, h, depth, shift, intra) in ((2, 64, 48, 2, 1, 1), (4, 64, 48, 3, 0, 0), (2, 16, 16, 3, 1, 1), (2, 64, 48, 2, 1, 0),
                                           (4, 8, 8, 3, 1, 1)):
        for queue in (0, 1, 0):
            walk.add("frame_histograms", OK, [depth, 0 if intra else 1, w, h, w >> shift, h >> shift, queue]
                     + frame(b, shift, shift, w, h, 2 * b), ["420" if shift else "444"])
    walk.add("frame_histograms", OK, [2, 0, 64, 48, 32, 48, 0] + frame(2, 1, 0, 64, 48), ["422"])
    walk.add("frame_histograms", EINVAL, [7, 0, 64, 48, 32, 24, 0] + frame(2, 1, 1, 64, 48))
    walk.add("frame_histograms", EINVAL, [2, 0, 128, 48, 32, 24, 0] + frame(2, 1, 1, 64, 48))


# ---- the slice encoder ----------------------------------------------------------------------------------------------------

def lowdelay(walk, every):
    def call(P, npictures, pads=(0, 0, 0), skew=0, status=OK, bps=2, fmt=None):
        nbytes = P["slice_bytes_num"] * P["n_horiz_slices"] * P["n_vert_slices"] // max(P["slice_bytes_denom"], 1)
        ints = [bps, npictures, skew] + lowdelay_ints(P) + [max(nbytes, 1), nbytes, P["n_horiz_slices"] * P["n_vert_slices"]]
        for _ in range(npictures):
            for k in range(3):
                w, h = (P["iwt_luma_width"], P["iwt_luma_height"]) if k == 0 else (P["iwt_chroma_width"], P["iwt_chroma_height"])
                ints += [span(h, 2 * w, 2 * w + pads[k]), 2 * w + pads[k]]
        classes = [str(f) for f in (fmt or format_of(P),) if f]
        if status == OK and LK.leaves_lds(P):
            classes.append("spill")
        if npictures >= 3:
            classes.append("three_picture_batch")       # (a call's pictures share their geometry: not "unlike" to the host)
        walk.add("lowdelay_encode", status, ints, classes)

    for name in sorted(LK.CASES):
        call(LK.CASES[name][0], 1)
    assert LK.leaves_lds(LK.CASES["spill_2x2"][0]) and LK.leaves_lds(LK.CASES["spill_3x5_420"][0])
    call(LK.CASES[LK.SPILL_BATCH[0]][0], len(LK.SPILL_BATCH[1]))
    call(LK.span_case()[0], 1)
    call(LK.turns_case()[0], 1)         # 68 x 66 slices: diagonals longer than the serial launch has threads
    for n, draw in enumerate(TD.lowdelay_draws()):
        if n % every == 0 or LK.leaves_lds(draw["P"]):
            call(draw["P"], len(draw["kinds"]), draw["pads"], draw["skew"], fmt=draw["fmt"])
    # the chain (tests/test_gpu_encode_chain.py): the forward transform in front of the slice encoder, planes and frame
    for n, draw in enumerate(TD.chain_draws()):
        P, depth, filt = draw["P"], draw["depth"], draw["filt"]
        hs, vs = FORMATS[draw["fmt"]]
        sizes = [(P["iwt_luma_width"], P["iwt_luma_height"])] + [(P["iwt_chroma_width"], P["iwt_chroma_height"])] * 2
        ints = [depth, filt, 2, 3]
        for (w, h), pad in zip(sizes, draw["pads"]):
            ints += [span(h, 2 * w, 2 * w), 2 * w, span(h, 2 * w, 2 * w + pad), 2 * w + pad, w, h]
        walk.add("iwt", OK, ints, ["iwt_out_of_place", "iwt_filter_%d" % filt, "iwt_depth_%d" % depth])
        call(P, 1, draw["pads"], fmt=draw["fmt"])
        fw, fh = max(sizes[0][0], sizes[1][0] << hs), max(sizes[0][1], sizes[1][1] << vs)
        nbytes = P["slice_bytes_num"] * P["n_horiz_slices"] * P["n_vert_slices"] // P["slice_bytes_denom"]
        walk.add("frame_iwt", OK, [1, depth, filt] + [v for s in sizes[:2] for v in s] + frame(2, hs, vs, fw, fh, draw["pads"][0]),
                 ["iwt_in_place", "iwt_filter_%d" % filt, "iwt_depth_%d" % depth, str(draw["fmt"])])
        walk.add("frame_lowdelay_encode", OK, lowdelay_ints(P) + [nbytes] + frame(2, hs, vs, fw, fh, draw["pads"][0]),
                 [str(draw["fmt"])] + (["spill"] if LK.leaves_lds(P) else []))
    # tests/test_gpu_lowdelay_encode.py::test_refusals: s32, then the parameters -- the chroma LL mismatch, the denominators
    # and the two size refusals -- over the buffers of the good geometry
    P = LK.CASES[LK.REFUSED_CASE][0]
    call(P, 1, status=EINVAL, bps=4)
    for word, bad in LK.refused_params(P):
        nbytes = P["slice_bytes_num"] * P["n_horiz_slices"] * P["n_vert_slices"] // P["slice_bytes_denom"]
        # (slices_bytes and the strides are what the changed parameters ask for: nothing but the change itself refuses the
        # call -- the planes are never touched by the host)
        claimed = bad["slice_bytes_num"] * bad["n_horiz_slices"] * bad["n_vert_slices"] // bad["slice_bytes_denom"] if bad["slice_bytes_denom"] > 0 else nbytes
        assert claimed <= nbytes
        ints = [2, 1, 0] + lowdelay_ints(bad) + [nbytes, claimed, P["n_horiz_slices"] * P["n_vert_slices"]]
        for k in range(3):
            w, h = (P["iwt_luma_width"], P["iwt_luma_height"]) if k == 0 else (P["iwt_chroma_width"], P["iwt_chroma_height"])
            ints += [span(h, 2 * w, 2 * w), max(2 * w, 2 * (bad["iwt_chroma_width"] if k else bad["iwt_luma_width"]))]
        walk.add("lowdelay_encode", EINVAL, ints, ["refused_" + word.replace(" ", "_")])
    hs, vs = shifts_of(P)
    nbytes = P["slice_bytes_num"] * P["n_horiz_slices"] * P["n_vert_slices"] // P["slice_bytes_denom"]
    walk.add("frame_lowdelay_encode", EINVAL, lowdelay_ints(P) + [nbytes] + frame(4, hs, vs, P["iwt_luma_width"], P["iwt_luma_height"]))
    walk.add("frame_lowdelay_encode", EINVAL, lowdelay_ints(dict(P, iwt_luma_width=2 * P["iwt_luma_width"])) + [nbytes]
             + frame(2, hs, vs, P["iwt_luma_width"], P["iwt_luma_height"]))


def build(thin=1):
    """(lines, classes).  thin = k keeps every k-th random draw (and every named case, every refusal, every draw on the
    spill path): the ThreadSanitizer build walks the file on three threads at once."""
    walk = Walk()
    analysis(walk, max(24 // thin, 4))
    rough(walk, thin)
    forward(walk, max(24 // thin, 4))
    residual(walk)
    quantise(walk, thin)
    histogram(walk, thin)
    lowdelay(walk, thin)
    return walk.lines, walk.classes
