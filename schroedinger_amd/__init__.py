"""schroedinger_amd -- MI355X (gfx950) execution domain for the Dirac/VC-2 decode
pixel path (inverse wavelet -> half-pel upsample -> OBMC + residual add).

The product is libschro_hip.so (C ABI: include/schro_hip.h; kernels:
schroedinger_amd/csrc/*.hip).  This package is only the thin Python view of
that ABI used by tests/ and bench.py: device planes, batched launches and the
SchroFrame-shaped stage calls.  No CPU fallback exists: every operator calls
the HIP library or raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SchroHipError, check  # noqa: F401

# SchroFrameFormat values, schroedinger/schroframe.h:22-35
FORMAT_U8_444, FORMAT_U8_422, FORMAT_U8_420 = 0x00, 0x01, 0x03
FORMAT_S16_444, FORMAT_S16_422, FORMAT_S16_420 = 0x04, 0x05, 0x07
FORMAT_S32_444, FORMAT_S32_422, FORMAT_S32_420 = 0x08, 0x09, 0x0b
FORMAT_YUYV, FORMAT_UYVY, FORMAT_AYUV = 0x100, 0x101, 0x102       # packed, schroframe.h:36-38
FORMAT_ARGB, FORMAT_V216, FORMAT_AY64 = 0x103, 0x105, 0x107
FORMAT_V210 = 0x106



def unpack_row_bytes(fmt, width):
    """Bytes of a packed row the unpack reads (schrovirtframe.c:616-893): YUYV / UYVY width / 2 four-byte groups, AYUV 4
    bytes per pixel, v216 8 bytes per pixel pair, v210 16 bytes per 6 pixels (the last group whole), AY64 8 per pixel."""
    return {FORMAT_YUYV: 4 * (width // 2), FORMAT_UYVY: 4 * (width // 2), FORMAT_AYUV: 4 * width,
            FORMAT_V216: 8 * (width // 2), FORMAT_V210: 16 * (-(-width // 6)), FORMAT_AY64: 8 * width}[fmt]


# SchroMotionVector, schroedinger/schromotion.h:20-37 (20 bytes)
MV_DTYPE = np.dtype([("flags", "<u4"), ("metric", "<u4"), ("chroma_metric", "<u4"),
                     ("v", "<i2", (4,))])


# SchroHipMetricScan / SchroHipMetricScanResult (include/schro_hip.h) as numpy records
SCAN_DTYPE = np.dtype([(n, "<i4") for n in ("x", "y", "block_width", "block_height", "ref_x", "ref_y", "scan_width", "scan_height",
                                            "gravity_x", "gravity_y", "dx", "dy")])
SCAN_RESULT_DTYPE = np.dtype([("dx", "<i4"), ("dy", "<i4"), ("metric", "<u4"), ("reserved", "<u4")])
LIMIT_METRIC_SCAN = 42


def metric_scan_setup(x, y, block_width, block_height, frame_width, frame_height, extension, dx, dy, dist):
    """schro_metric_scan_setup (schrometric.c:174-214) on the host: (ref_x, ref_y, scan_width, scan_height) of the window
    of `dist` around (x + dx, y + dy); the sizes may come out <= 0.  Raises where the reference asserts."""
    s = _lib.MetricScan(x=x, y=y, block_width=block_width, block_height=block_height)
    check(_lib.load().schro_hip_metric_scan_setup(C.byref(s), frame_width, frame_height, extension, dx, dy, dist))
    return s.ref_x, s.ref_y, s.scan_width, s.scan_height


def lowpass2_coeff(sigma):
    """generate_coeff (schrofilter.c:666-689) on the host (schro_hip_lowpass2_coeff): the four doubles of one sigma."""
    c = (C.c_double * 4)()
    _lib.load().schro_hip_lowpass2_coeff(float(sigma), c)
    return [float(v) for v in c]


PICTURE_STATS_GEOMETRY = ("sums_tile_bytes", "sums_tile_rows", "lowpass_rows", "lowpass_chunk", "lowpass_cols", "lowpass_col_rows",
                          "ssim_tile_cols", "ssim_tile_rows")


def picture_stats_geometry():
    """{name: length} of the tiles and chunks of the picture-statistics kernels, from the library
    (schro_hip_picture_stats_geometry): the sizes around which the tests place their planes."""
    v = (C.c_int * len(PICTURE_STATS_GEOMETRY))()
    _lib.load().schro_hip_picture_stats_geometry(v)
    return dict(zip(PICTURE_STATS_GEOMETRY, (int(x) for x in v)))


UNPACK_GEOMETRY = 58            # SCHRO_HIP_UNPACK_GEOMETRY (include/schro_hip.h)


def unpack_geometry():
    """The tile lengths of the encoder's way in, from the library (schro_hip_unpack_geometry): {"tile_bytes", "tile_rows":
    destination bytes of a row and rows of an unpack_batch tile; "iwt": {(filter, bytes per sample): (useful column pairs,
    useful row pairs, halo column pairs, halo row pairs) of the forward wavelet's tile}}."""
    v = (C.c_int * UNPACK_GEOMETRY)()
    _lib.load().schro_hip_unpack_geometry(v)
    iwt = {(f, bpp): tuple(int(x) for x in v[2 + 4 * (2 * f + b):6 + 4 * (2 * f + b)]) for f in range(7) for b, bpp in enumerate((2, 4))}
    return dict(tile_bytes=int(v[0]), tile_rows=int(v[1]), iwt=iwt)


SSIM_RESULT_DTYPE = np.dtype([("sum", "<f8"), ("out_of_range", "<u4", (5,)), ("reserved", "<u4")])


def _coeff4(v):
    return lowpass2_coeff(v) if np.isscalar(v) else [float(x) for x in v]


def sums_jobs(jobs):
    """The SchroHipSumsJob array of Context.plane_sums_batch's jobs: (a, b or None, result) per job."""
    arr = (_lib.SumsJob * len(jobs))()
    for j, (a, b, result) in zip(arr, jobs):
        j.a, j.a_stride, j.bytes_per_sample, j.width, j.height = a.ptr, a.stride, np.dtype(a.dtype).itemsize, a.width, a.height
        if b is not None:
            j.b, j.b_stride, j.b_width, j.b_height = b.ptr, b.stride, b.width, b.height
        j.result = result.ptr
    return arr


def lowpass2_planes(planes):
    """The SchroHipLowpass2Plane array of Context.lowpass2_batch's planes: (plane, h, v, counter) per plane -- h, v: a sigma
    or four coefficients."""
    arr = (_lib.Lowpass2Plane * len(planes))()
    for p, (pl, h, v, counter) in zip(arr, planes):
        p.data, p.stride, p.bytes_per_sample, p.width, p.height = pl.ptr, pl.stride, np.dtype(pl.dtype).itemsize, pl.width, pl.height
        p.h_coeff[:], p.v_coeff[:] = _coeff4(h), _coeff4(v)
        p.out_of_range = counter.ptr
    return arr


def ssim_pictures(pictures):
    """The SchroHipSsimPicture array of Context.ssim_batch's pictures: (a, b, map or None, scratch, result) per picture --
    scratch: a span of bytes (.ptr, .width bytes)."""
    arr = (_lib.SsimPicture * len(pictures))()
    for p, (a, b, m, scratch, result) in zip(arr, pictures):
        p.a, p.a_stride, p.width, p.height = a.ptr, a.stride, a.width, a.height
        p.b, p.b_stride, p.b_width, p.b_height = b.ptr, b.stride, b.width, b.height
        p.scratch, p.scratch_bytes, p.result = scratch.ptr, scratch.width * np.dtype(scratch.dtype).itemsize, result.ptr
        if m is not None:
            p.map, p.map_stride = m.ptr, m.stride
    return arr


def plane_sums_check(jobs):
    """The refusals of Context.plane_sums_batch on the host, without a context (schro_hip_plane_sums_check)."""
    check(_lib.load().schro_hip_plane_sums_check(sums_jobs(jobs), len(jobs)))


def lowpass2_check(planes):
    """... of Context.lowpass2_batch (schro_hip_lowpass2_check)."""
    check(_lib.load().schro_hip_lowpass2_check(lowpass2_planes(planes), len(planes)))


def ssim_check(pictures):
    """... of Context.ssim_batch (schro_hip_ssim_check)."""
    check(_lib.load().schro_hip_ssim_check(ssim_pictures(pictures), len(pictures)))


def ssim_scratch_bytes(width, height):
    """schro_hip_ssim_scratch_bytes: the scratch one picture of Context.ssim_batch needs (0: no such picture)."""
    return int(_lib.load().schro_hip_ssim_scratch_bytes(width, height))


ROUGH_WAVES = 16                # SCHRO_HIP_ROUGH_WAVES (include/schro_hip.h): the most waves a rough-search workgroup has
MAX_HIER_LEVELS = _lib.MAX_HIER_LEVELS


def _block_geometry(params):
    return tuple(int(params[k] if isinstance(params, dict) else getattr(params, k))
                 for k in ("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"))


def rough_hint_pictures(pictures):
    """The SchroHipRoughHintPicture array of [(frame, ref, extension, params, shift, distance, ref_index, hint_field,
    field)]: frame, ref -- u8 planes of one size at level `shift` (anything with ptr, stride, width, height); params -- a
    dict (or _lib.Params) with x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma; hint_field, field -- device fields
    (Context.motion_field, or anything with ptr)."""
    arr = (_lib.RoughHintPicture * len(pictures))()
    for k, (f, r, ext, params, shift, dist, ref_index, hint, field) in enumerate(pictures):
        assert (f.height, f.width) == (r.height, r.width)
        arr[k] = _lib.RoughHintPicture(f.ptr, f.stride, r.ptr, r.stride, f.width, f.height, ext, *_block_geometry(params),
                                       shift, dist, ref_index, hint.ptr, field.ptr)
    return arr


def rough_chains(chains):
    """The SchroHipRoughChain array of [(levels, params, ref_index, fields)]: levels -- [(frame, ref, extension)] for
    pyramid levels 1 .. n_levels, fields -- the device field of each.  Returns (array, what it points to)."""
    arr, keep = (_lib.RoughChain * len(chains))(), []
    for k, (levels, params, ref_index, fields) in enumerate(chains):
        assert len(levels) == len(fields)
        n = len(levels)
        lv = (_lib.RoughPlane * max(n, 1))()
        for m, (f, r, ext) in enumerate(levels):
            assert (f.height, f.width) == (r.height, r.width)
            lv[m] = _lib.RoughPlane(f.ptr, f.stride, r.ptr, r.stride, f.width, f.height, ext)
        keep.append(lv)
        arr[k].n_levels, arr[k].levels = n, lv
        arr[k].x_num_blocks, arr[k].y_num_blocks, arr[k].xbsep_luma, arr[k].ybsep_luma = _block_geometry(params)
        arr[k].ref_index = ref_index
        for m, fld in enumerate(fields[:MAX_HIER_LEVELS]):
            arr[k].fields[m] = fld.ptr
    return arr, keep


def rough_hint_check(pictures):
    """The refusals of Context.rough_hint_batch on the host, without a context (schro_hip_rough_hint_check)."""
    check(_lib.load().schro_hip_rough_hint_check(rough_hint_pictures(pictures), len(pictures)))


def rough_me_check(chains, nohint_distance=12, hint_distance=4):
    """The refusals of Context.rough_me_batch on the host, without a context (schro_hip_rough_me_check)."""
    arr, keep = rough_chains(chains)
    check(_lib.load().schro_hip_rough_me_check(arr, len(chains), nohint_distance, hint_distance))


def _hbm_plane(frame, ref, ext, h_shift, v_shift):
    """The SchroHipHbmPlane of (Y, U, V) planes of a frame and of its reference at one level."""
    assert len(frame) == len(ref) == 3
    pl = _lib.HbmPlane()
    for k in range(3):
        assert (frame[k].height, frame[k].width) == (ref[k].height, ref[k].width)
        pl.frame[k], pl.frame_stride[k] = frame[k].ptr, frame[k].stride
        pl.ref[k], pl.ref_stride[k] = ref[k].ptr, ref[k].stride
    pl.width, pl.height, pl.h_shift, pl.v_shift, pl.extension = frame[0].width, frame[0].height, h_shift, v_shift, ext
    return pl


def hbm_levels(levels):
    """The SchroHipHbmLevel array of [(frame, ref, extension, h_shift, v_shift, params, shift, h_range, ref_index,
    hint_field, field)]: frame, ref -- the (Y, U, V) u8 planes at level `shift` (anything with ptr, stride, width, height);
    params -- a dict (or _lib.Params) with x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma; hint_field -- the device
    field of level shift + 1 or None, field -- the device field written (Context.motion_field, or anything with ptr)."""
    arr = (_lib.HbmLevel * len(levels))()
    for k, (f, r, ext, hs, vs, params, shift, h_range, ref_index, hint, field) in enumerate(levels):
        arr[k].plane = _hbm_plane(f, r, ext, hs, vs)
        arr[k].x_num_blocks, arr[k].y_num_blocks, arr[k].xbsep_luma, arr[k].ybsep_luma = _block_geometry(params)
        arr[k].shift, arr[k].h_range, arr[k].ref_index = shift, h_range, ref_index
        arr[k].hint_field, arr[k].field = (hint.ptr if hint is not None else None), field.ptr
    return arr


def hbm_chains(chains):
    """The SchroHipHbmChain array of [(levels, h_shift, v_shift, params, ref_index, fields)]: levels -- [(frame, ref,
    extension)] with (Y, U, V) planes for pyramid levels 0 .. n_levels, fields -- the device field of each; entry 0 of
    both may be None for a call without level 0.  Returns (array, what it points to)."""
    arr, keep = (_lib.HbmChain * len(chains))(), []
    for k, (levels, hs, vs, params, ref_index, fields) in enumerate(chains):
        assert len(levels) == len(fields)
        n = len(levels) - 1
        lv = (_lib.HbmPlane * max(n + 1, 1))()
        for m, t in enumerate(levels):
            if t is not None:
                lv[m] = _hbm_plane(t[0], t[1], t[2], hs, vs)
        keep.append(lv)
        arr[k].n_levels, arr[k].levels = n, lv
        arr[k].x_num_blocks, arr[k].y_num_blocks, arr[k].xbsep_luma, arr[k].ybsep_luma = _block_geometry(params)
        arr[k].ref_index = ref_index
        for m, fld in enumerate(fields[:MAX_HIER_LEVELS + 1]):
            arr[k].fields[m] = fld.ptr if fld is not None else None
    return arr, keep


def hbm_level_check(levels):
    """The refusals of Context.hbm_level_batch on the host, without a context (schro_hip_hbm_level_check)."""
    check(_lib.load().schro_hip_hbm_level_check(hbm_levels(levels), len(levels)))


def hbm_check(chains, with_level0=True):
    """The refusals of Context.hbm_batch on the host, without a context (schro_hip_hbm_check)."""
    arr, keep = hbm_chains(chains)
    check(_lib.load().schro_hip_hbm_check(arr, len(chains), int(bool(with_level0))))


def subpel_chains(chains):
    """The SchroHipSubpelChain array of [(src, ref_up, extension, params, mv_precision, ref_index, lambda, src_field,
    field)]: src -- the u8 luma plane of the picture (anything with ptr, stride, width, height); ref_up -- the tiled
    upsampled luma image of the reference (Context.hp_plane, or anything with ptr, stride); params -- a dict (or
    _lib.Params) with x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma; src_field, field -- device fields
    (Context.motion_field, or anything with ptr; they may be one); src_field may be None for the single-pass calls."""
    arr = (_lib.SubpelChain * len(chains))()
    for k, (src, up, ext, params, prec, ref_index, lam, src_field, field) in enumerate(chains):
        a = arr[k]
        a.src, a.src_stride, a.ref_up, a.ref_up_stride = src.ptr, src.stride, up.ptr, up.stride
        a.width, a.height, a.extension = src.width, src.height, ext
        a.x_num_blocks, a.y_num_blocks, a.xbsep_luma, a.ybsep_luma = _block_geometry(params)
        a.mv_precision, a.ref_index = prec, ref_index
        setattr(a, "lambda", float(lam))
        a.src_field, a.field = (src_field.ptr if src_field is not None else None), field.ptr
    return arr


def subpel_check(chains):
    """The refusals of Context.subpel_batch on the host, without a context (schro_hip_subpel_check)."""
    check(_lib.load().schro_hip_subpel_check(subpel_chains(chains), len(chains)))


def _subpel_tables(tables):
    arr = (C.c_void_p * len(tables))()
    for k, t in enumerate(tables):
        arr[k] = t.ptr
    return arr


SB_DTYPE = np.dtype([("error", "<i4"), ("entropy", "<i4"), ("score", "<f8")])    # a superblock of the split-2 mode decision
SPLIT2_TABLE_INTS = 16          # SCHRO_HIP_SPLIT2_TABLE_INTS (include/schro_hip.h)


def split2_pictures(pictures):
    """The SchroHipSplit2Picture array of [(src, refs, shifts, extension, params, lambda, fields, motion, superblocks)]:
    src -- the Y, U, V planes of the picture, linear u8 (anything with ptr, stride, width, height; entries may be None
    only to be refused); refs -- per reference the tiled upsampled images of Y, U, V (Context.hp_plane, or anything with
    ptr, stride); shifts -- (h_shift, v_shift); params -- a dict with x_num_blocks, y_num_blocks, xbsep_luma, ybsep_luma
    and mv_precision; fields -- per reference the device sub-pel field; motion, superblocks -- device memory for 20 bytes
    per block and 16 per superblock (Context.motion_field, or anything with ptr)."""
    arr = (_lib.Split2Picture * len(pictures))()
    for n, (src, refs, shifts, ext, params, lam, fields, motion, superblocks) in enumerate(pictures):
        a = arr[n]
        for k in range(3):
            if src[k] is not None:
                a.src[k], a.src_stride[k] = src[k].ptr, src[k].stride
        a.width, a.height = src[0].width, src[0].height
        a.num_refs = len(refs)
        for r, ups in enumerate(refs[:2]):
            for k in range(3):
                if ups[k] is not None:
                    a.ref_up[r][k], a.ref_up_stride[k] = ups[k].ptr, ups[k].stride
        a.h_shift, a.v_shift = shifts
        a.extension = ext
        a.x_num_blocks, a.y_num_blocks, a.xbsep_luma, a.ybsep_luma = _block_geometry(params)
        a.mv_precision = params["mv_precision"]
        setattr(a, "lambda", float(lam))
        for r, f in enumerate(fields[:2]):
            a.fields[r] = f.ptr if f is not None else None
        a.motion = motion.ptr if motion is not None else None
        a.superblocks = superblocks.ptr if superblocks is not None else None
    return arr


def split2_check(pictures):
    """The refusals of Context.split2_batch on the host, without a context (schro_hip_split2_check)."""
    check(_lib.load().schro_hip_split2_check(split2_pictures(pictures), len(pictures)))


MODE_TABLE_INTS = 532           # SCHRO_HIP_MODE_TABLE_INTS (include/schro_hip.h): per superblock
MODE_CANDIDATES, MODE_CANDIDATE_INTS, MODE_ZERO_TRIAL = 22, 12, 528     # per reference 22 candidates of 12 int32; the zero-vector trial
# a trial of a superblock (SchroHipModeTrial): four per superblock -- split 2, split 1, split 0, the zero vectors
MODE_TRIAL_DTYPE = np.dtype([("state", "<i4"), ("error", "<i4"), ("entropy", "<i4"), ("pad", "<i4"), ("score", "<f8")])


def mode_pictures(pictures):
    """The SchroHipModePicture array of [(src, refs, shifts, extension, params, lambda, fields, level1, level2, motion,
    superblocks, trials, stats)]: as split2_pictures takes them, and level1, level2 -- per reference the device level-1
    and level-2 field of the block matching; trials -- device memory for four MODE_TRIAL_DTYPE per superblock; stats --
    device memory for three doubles."""
    arr = (_lib.ModePicture * len(pictures))()
    for n, (src, refs, shifts, ext, params, lam, fields, level1, level2, motion, superblocks, trials, stats) in enumerate(pictures):
        one = split2_pictures([(src, refs, shifts, ext, params, lam, fields, motion, superblocks)])
        C.memmove(C.byref(arr[n].split2), one, C.sizeof(_lib.Split2Picture))
        for r in range(min(len(refs), 2)):
            for level, f in enumerate((level1, level2)):
                arr[n].hbm_fields[r][level] = f[r].ptr if r < len(f) and f[r] is not None else None
        arr[n].trials = trials.ptr if trials is not None else None
        arr[n].stats = stats.ptr if stats is not None else None
    return arr


def mode_check(pictures):
    """The refusals of Context.mode_decision_batch on the host, without a context (schro_hip_mode_decision_check)."""
    check(_lib.load().schro_hip_mode_decision_check(mode_pictures(pictures), len(pictures)))


def noarith_pictures(pictures):
    """The SchroHipNoarithPicture array of [(planes, tables, depth, horiz_codeblocks, vert_codeblocks, codeblock_mode_index,
    out, capacity, result)]: planes -- the Y, U, V quant planes at the transform's size (anything with ptr, stride, width,
    height); tables -- per component the C table of Context.codeblock_layout for that plane's stride with the quant
    indices filled in (or a list of record tuples); out, result -- device memory (anything with ptr) or None.  Returns
    (array, what it points to)."""
    arr = (_lib.NoarithPicture * len(pictures))()
    keep = []
    for a, (planes, tables, depth, hc, vc, mode, out, capacity, result) in zip(arr, pictures):
        for k in range(3):
            tab = tables[k] if isinstance(tables[k], C.Array) else Context.codeblock_table(tables[k])
            keep.append(tab)
            a.quant[k], a.stride[k] = planes[k].ptr, planes[k].stride
            a.iwt_width[k], a.iwt_height[k] = planes[k].width, planes[k].height
            a.bytes[k] = planes[k].stride * planes[k].height
            a.codeblocks[k], a.ncodeblocks[k] = tab, len(tab)
        a.transform_depth, a.codeblock_mode_index = depth, mode
        for l in range(min(len(hc), 7)):
            a.horiz_codeblocks[l], a.vert_codeblocks[l] = hc[l], vc[l]
        a.out = out.ptr if out is not None else None
        a.capacity = capacity
        a.result = result.ptr if result is not None else None
    return arr, keep


def noarith_encode_check(pictures, bpp):
    """The refusals of Context.noarith_encode_batch on the host, without a context (schro_hip_noarith_encode_check)."""
    arr, keep = noarith_pictures(pictures)
    check(_lib.load().schro_hip_noarith_encode_check(arr, len(pictures), bpp))


def noarith_encode_chosen_check(pictures, chosen, clamped, bpp):
    """The refusals of Context.noarith_encode_chosen_batch on the host, without a context."""
    arr, keep = noarith_pictures(pictures)
    ptrs = (C.c_void_p * max(len(chosen), 1))(*[getattr(c, "ptr", c) for c in chosen])
    check(_lib.load().schro_hip_noarith_encode_chosen_check(arr, ptrs, len(pictures), bpp, getattr(clamped, "ptr", clamped)))


def noarith_encode_bound(sizes, depth, horiz_codeblocks, vert_codeblocks, bpp):
    """schro_hip_noarith_encode_bound: the output capacity that always suffices for a picture whose components are
    sizes = [(width, height)] * 3 at the transform's size."""
    a = _lib.NoarithPicture()
    for k, (w, h) in enumerate(sizes):
        a.iwt_width[k], a.iwt_height[k] = w, h
    a.transform_depth = depth
    for l in range(min(len(horiz_codeblocks), 7)):
        a.horiz_codeblocks[l], a.vert_codeblocks[l] = horiz_codeblocks[l], vert_codeblocks[l]
    n = _lib.load().schro_hip_noarith_encode_bound(C.byref(a), bpp)
    if n < 0:
        check(int(n))
    return int(n)


def noarith_result(words):
    """A downloaded SchroHipNoarithResult (uint32 words) as a dict: bytes, overrun, false_zero (codeblocks, sub-bands),
    subband_bits (3 x 19)."""
    w = np.asarray(words, np.uint32).ravel()
    return {"bytes": int(w[0]), "overrun": int(w[1]), "false_zero": (int(w[2]), int(w[3])),
            "subband_bits": w[4:4 + 3 * _lib.NOARITH_MAX_SUBBANDS].astype(np.int64).reshape(3, _lib.NOARITH_MAX_SUBBANDS)}


def noarith_decode_pictures(pictures):
    """The SchroHipNoarithDecodePicture array of [(data, data_bytes, bytes_on_device, coeffs, quant, depth, horiz_codeblocks,
    vert_codeblocks, codeblock_mode_index, is_intra, compat_quant_offset, result)]: data, bytes_on_device, result -- device
    memory (anything with ptr, or an address) or None; coeffs -- the Y, U, V planes at the transform's size (anything with
    ptr, stride, width, height); quant -- three planes of the same layout or None."""
    return _fill_decode_pictures((_lib.NoarithDecodePicture * len(pictures))(), pictures)


def _fill_decode_pictures(arr, pictures):
    """The fields the VLC and the arithmetic decode pictures share."""
    addr = lambda m: None if m is None else getattr(m, "ptr", m)
    for a, (data, nbytes, on_device, coeffs, quant, depth, hc, vc, mode, is_intra, compat, result) in zip(arr, pictures):
        a.data, a.data_bytes, a.bytes_on_device = addr(data), nbytes, addr(on_device)
        for k in range(3):
            a.coeffs[k], a.stride[k] = coeffs[k].ptr, coeffs[k].stride
            a.iwt_width[k], a.iwt_height[k] = coeffs[k].width, coeffs[k].height
            a.bytes[k] = coeffs[k].stride * coeffs[k].height
            a.quant[k] = quant[k].ptr if quant is not None else None
        a.transform_depth, a.codeblock_mode_index = depth, mode
        for l in range(min(len(hc), 7)):
            a.horiz_codeblocks[l], a.vert_codeblocks[l] = hc[l], vc[l]
        a.is_intra, a.compat_quant_offset = int(bool(is_intra)), int(bool(compat))
        a.result = addr(result)
    return arr


def noarith_decode_check(pictures, bpp):
    """The refusals of Context.noarith_decode_batch on the host, without a context (schro_hip_noarith_decode_check)."""
    check(_lib.load().schro_hip_noarith_decode_check(noarith_decode_pictures(pictures), len(pictures), bpp))


def noarith_decode_result(words):
    """A downloaded SchroHipNoarithDecodeResult (uint32 words, or the ctypes structure) as a dict: bytes_read, error,
    first_error, compat_quant_offset, truncated, not_consumed, overran, long_codes, clamped_quant, subband_length (3 x 19),
    subband_quant_index (3 x 19)."""
    if isinstance(words, _lib.NoarithDecodeResult):
        words = np.frombuffer(bytes(words), np.uint32)
    w = np.ascontiguousarray(np.asarray(words, np.uint32).ravel()[:C.sizeof(_lib.NoarithDecodeResult) // 4])
    n = 3 * _lib.NOARITH_MAX_SUBBANDS
    names = ("bytes_read", "error", "first_error", "compat_quant_offset", "truncated", "not_consumed", "overran", "long_codes",
             "clamped_quant")
    out = {k: int(v) for k, v in zip(names, w[:9])}
    out["subband_length"] = w[9:9 + n].astype(np.int64).reshape(3, _lib.NOARITH_MAX_SUBBANDS)
    out["subband_quant_index"] = w[9 + n:].view(np.uint8)[:n].astype(np.int64).reshape(3, _lib.NOARITH_MAX_SUBBANDS)
    return out


def arith_decode_pictures(pictures):
    """The SchroHipArithDecodePicture array of the twelve entries noarith_decode_pictures takes, with the same meanings."""
    return _fill_decode_pictures((_lib.ArithDecodePicture * len(pictures))(), pictures)


def arith_decode_check(pictures, bpp):
    """The refusals of Context.arith_decode_batch on the host, without a context (schro_hip_arith_decode_check)."""
    check(_lib.load().schro_hip_arith_decode_check(arith_decode_pictures(pictures), len(pictures), bpp))


def arith_decode_scratch_words(pictures, bpp):
    """The words of queue scratch Context.arith_decode_batch takes for these pictures (schro_hip_arith_decode_scratch_words)."""
    n = int(_lib.load().schro_hip_arith_decode_scratch_words(arith_decode_pictures(pictures), len(pictures), bpp))
    if n < 0:
        check(n)
    return n


def arith_decode_result(words):
    """A downloaded SchroHipArithDecodeResult (uint32 words, or the ctypes structure) as a dict: the entries of
    noarith_decode_result with the arithmetic decoder's meanings, and bins."""
    if isinstance(words, _lib.ArithDecodeResult):
        words = np.frombuffer(bytes(words), np.uint32)
    w = np.ascontiguousarray(np.asarray(words, np.uint32).ravel()[:C.sizeof(_lib.ArithDecodeResult) // 4])
    out = noarith_decode_result(w)
    out["bins"] = int(w[_lib.ArithDecodeResult.bins.offset // 4])
    return out


def motion_encode_pictures(pictures):
    """The SchroHipMotionEncodePicture array of [(motion, x_num_blocks, y_num_blocks, num_refs, have_global_motion, out,
    capacity, result)]: motion, out, result -- device memory (anything with ptr, or an address) or None."""
    arr = (_lib.MotionEncodePicture * len(pictures))()
    addr = lambda m: None if m is None else getattr(m, "ptr", m)
    for a, (motion, nbx, nby, num_refs, hg, out, capacity, result) in zip(arr, pictures):
        a.motion, a.x_num_blocks, a.y_num_blocks, a.num_refs, a.have_global_motion = addr(motion), nbx, nby, num_refs, int(hg)
        a.out, a.capacity, a.result = addr(out), capacity, addr(result)
    return arr


def motion_encode_check(pictures):
    """The refusals of Context.motion_encode_batch on the host, without a context (schro_hip_motion_encode_check)."""
    check(_lib.load().schro_hip_motion_encode_check(motion_encode_pictures(pictures), len(pictures)))


def motion_encode_bound(x_num_blocks, y_num_blocks, num_refs, have_global_motion):
    """schro_hip_motion_encode_bound: the output capacity that always suffices for a picture's motion data."""
    n = _lib.load().schro_hip_motion_encode_bound(x_num_blocks, y_num_blocks, num_refs, int(have_global_motion))
    if n < 0:
        check(int(n))
    return int(n)


def motion_encode_result(words):
    """A downloaded SchroHipMotionEncodeResult (uint32 words) as a dict: bytes, overrun, section_bytes (9), section_units
    (9), asserted, unverified, first_unverified."""
    w = np.asarray(words, np.uint32).ravel()
    n = _lib.MOTION_SECTIONS
    return {"bytes": int(w[0]), "overrun": int(w[1]), "section_bytes": [int(x) for x in w[2:2 + n]],
            "section_units": [int(x) for x in w[2 + n:2 + 2 * n]], "asserted": int(w[2 + 2 * n]), "unverified": int(w[3 + 2 * n]),
            "first_unverified": int(w[4 + 2 * n:5 + 2 * n].view(np.int32)[0])}


def motion_decode_pictures(pictures):
    """The SchroHipMotionDecodePicture array of [(data, data_bytes, bytes_on_device, x_num_blocks, y_num_blocks, num_refs,
    have_global_motion, motion, result)]: data, bytes_on_device, motion, result -- device memory (anything with ptr, or an
    address) or None."""
    arr = (_lib.MotionDecodePicture * len(pictures))()
    addr = lambda m: None if m is None else getattr(m, "ptr", m)
    for a, (data, data_bytes, word, nbx, nby, num_refs, hg, motion, result) in zip(arr, pictures):
        a.data, a.data_bytes, a.bytes_on_device = addr(data), data_bytes, addr(word)
        a.x_num_blocks, a.y_num_blocks, a.num_refs, a.have_global_motion = nbx, nby, num_refs, int(hg)
        a.motion, a.result = addr(motion), addr(result)
    return arr


def motion_decode_check(pictures):
    """The refusals of Context.motion_decode_batch on the host, without a context (schro_hip_motion_decode_check)."""
    check(_lib.load().schro_hip_motion_decode_check(motion_decode_pictures(pictures), len(pictures)))


def motion_decode_scratch_words(pictures):
    """schro_hip_motion_decode_scratch_words: the words of queue scratch Context.motion_decode_batch takes."""
    n = _lib.load().schro_hip_motion_decode_scratch_words(motion_decode_pictures(pictures), len(pictures))
    if n < 0:
        check(int(n))
    return int(n)


def motion_decode_result(words):
    """A downloaded SchroHipMotionDecodeResult (uint32 words) as a dict: bytes, section_bytes (9), section_units (9),
    section_bits (9), truncated, overran, not_consumed (masks over sections), long_codes, unverified, first_unverified."""
    w = np.asarray(words, np.uint32).ravel()
    n = _lib.MOTION_SECTIONS
    return {"bytes": int(w[0]), "section_bytes": [int(x) for x in w[1:1 + n]], "section_units": [int(x) for x in w[1 + n:1 + 2 * n]],
            "section_bits": [int(x) for x in w[1 + 2 * n:1 + 3 * n]], "truncated": int(w[1 + 3 * n]), "overran": int(w[2 + 3 * n]),
            "not_consumed": int(w[3 + 3 * n]), "long_codes": int(w[4 + 3 * n]), "unverified": int(w[5 + 3 * n]),
            "first_unverified": int(w[6 + 3 * n:7 + 3 * n].view(np.int32)[0])}


def motion_arith_decode_pictures(pictures):
    """The SchroHipMotionArithDecodePicture array of [(data, data_bytes, bytes_on_device, x_num_blocks, y_num_blocks,
    num_refs, have_global_motion, motion, result)], as motion_decode_pictures takes them."""
    arr = (_lib.MotionArithDecodePicture * len(pictures))()
    addr = lambda m: None if m is None else getattr(m, "ptr", m)
    for a, (data, data_bytes, word, nbx, nby, num_refs, hg, motion, result) in zip(arr, pictures):
        a.data, a.data_bytes, a.bytes_on_device = addr(data), data_bytes, addr(word)
        a.x_num_blocks, a.y_num_blocks, a.num_refs, a.have_global_motion = nbx, nby, num_refs, int(hg)
        a.motion, a.result = addr(motion), addr(result)
    return arr


def motion_arith_decode_check(pictures):
    """The refusals of Context.motion_arith_decode_batch on the host, without a context
    (schro_hip_motion_arith_decode_check)."""
    check(_lib.load().schro_hip_motion_arith_decode_check(motion_arith_decode_pictures(pictures), len(pictures)))


def motion_arith_decode_scratch_words(pictures):
    """schro_hip_motion_arith_decode_scratch_words: the words of queue scratch Context.motion_arith_decode_batch takes."""
    n = _lib.load().schro_hip_motion_arith_decode_scratch_words(motion_arith_decode_pictures(pictures), len(pictures))
    if n < 0:
        check(int(n))
    return int(n)


def motion_arith_decode_result(words):
    """A downloaded SchroHipMotionArithDecodeResult (uint32 words) as a dict: bytes, section_bytes, section_units,
    section_offset, section_bins (9 each), truncated, overran, not_consumed (masks over sections), long_codes, unverified,
    first_unverified."""
    w = np.asarray(words, np.uint32).ravel()
    n = _lib.MOTION_SECTIONS
    return {"bytes": int(w[0]), "section_bytes": [int(x) for x in w[1:1 + n]], "section_units": [int(x) for x in w[1 + n:1 + 2 * n]],
            "section_offset": [int(x) for x in w[1 + 2 * n:1 + 3 * n]], "section_bins": [int(x) for x in w[1 + 3 * n:1 + 4 * n]],
            "truncated": int(w[1 + 4 * n]), "overran": int(w[2 + 4 * n]), "not_consumed": int(w[3 + 4 * n]),
            "long_codes": int(w[4 + 4 * n]), "unverified": int(w[5 + 4 * n]),
            "first_unverified": int(w[6 + 4 * n:7 + 4 * n].view(np.int32)[0])}


# SchroHipQuantChoice (include/schro_hip.h) as a numpy record
QUANT_CHOICE_DTYPE = np.dtype([("frame_lambda", "<f8"), ("sum", "<f8"), ("chosen_entropy", "<f8", (3, _lib.QUANT_CHOOSE_BANDS)),
                               ("chosen_error", "<f8", (3, _lib.QUANT_CHOOSE_BANDS)), ("quant_index", "<i4", (3, _lib.QUANT_CHOOSE_BANDS)),
                               ("evaluations", "<i4"), ("not_bracketed", "<i4"), ("reserved", "<i4")])
QUANT_ENGINE_LAMBDA, QUANT_ENGINE_BIT_ALLOCATION, QUANT_ENGINE_CONSTANT_ERROR = 0, 1, 2


def quant_choose_pictures(pictures):
    """The SchroHipQuantChoosePicture array of a list of dicts: counts (three device arrays of SchroHipHistogramCounts:
    anything with ptr, or an address), skip (per sub-band), depth, is_intra, is_noarith, engine, weight (per sub-band),
    ratio ([3][sub-bands]), scales (sub-band 0, chroma, diagonal), target, result and optionally est_entropy, est_error
    (device memory, as counts)."""
    arr = (_lib.QuantChoosePicture * len(pictures))()
    addr = lambda m: None if m is None else getattr(m, "ptr", m)
    for a, p in zip(arr, pictures):
        for c in range(3):
            a.counts[c] = addr(p["counts"][c])
        for i, s in enumerate(p["skip"]):
            a.skip[i] = int(s)
        a.transform_depth, a.is_intra, a.is_noarith, a.engine = int(p["depth"]), int(p["is_intra"]), int(p["is_noarith"]), int(p["engine"])
        for i, w in enumerate(list(p["weight"])[:_lib.QUANT_CHOOSE_BANDS]):
            a.subband_weight[i] = float(w)
        for c in range(3):
            for i, r in enumerate(list(p["ratio"][c])[:_lib.QUANT_CHOOSE_BANDS]):
                a.context_ratio[c][i] = float(r)
        a.subband0_lambda_scale, a.chroma_lambda_scale, a.diagonal_lambda_scale = (float(s) for s in p["scales"])
        a.target = float(p["target"])
        a.result, a.est_entropy, a.est_error = addr(p["result"]), addr(p.get("est_entropy")), addr(p.get("est_error"))
    return arr


def quant_choose_check(pictures, have_bit_tables=True):
    """The refusals of Context.quant_choose_batch on the host, without a context (schro_hip_quant_choose_check)."""
    check(_lib.load().schro_hip_quant_choose_check(quant_choose_pictures(pictures), len(pictures), 1 if have_bit_tables else 0))


QUANTISE_DC_THREADS = 256      # SCHRO_HIP_QUANTISE_DC_THREADS (include/schro_hip.h): the DC recurrence's workgroup size


def device_count():
    return _lib.load().schro_hip_device_count()


class DevicePlane:
    """A 2-D array in the context's memory domain."""

    def __init__(self, ctx, height, width, dtype, stride=None):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self.height, self.width = int(height), int(width)
        row = self.width * self.dtype.itemsize
        self.stride = int(stride) if stride else (row + 63) // 64 * 64
        self.nbytes = self.stride * self.height
        self.ptr = ctx.alloc(self.nbytes)

    def level_view(self, level=1):
        """The level-`level` view of a coefficient plane in the reference's in-place layout (schroparams.c:319-352): the
        same memory, {width >> level, height >> level, stride << level} -- the `src` of a call that runs only the levels
        from `level` up (Context.iiwt_batch)."""
        v = DevicePlane.__new__(DevicePlane)
        v.ctx, v.dtype = self.ctx, self.dtype
        v.height, v.width, v.stride = self.height >> level, self.width >> level, self.stride << level
        v.nbytes, v.ptr = 0, self.ptr
        v.free = lambda: None           # (the memory is the parent's)
        return v

    def rows_view(self, first, count):
        """Rows first .. first + count - 1 as a plane of their own: the same memory, upload () / download () work on it,
        free () does nothing (the memory is the parent's)."""
        assert 0 <= first and count >= 0 and first + count <= self.height
        v = self.level_view(0)
        v.height, v.nbytes, v.ptr = int(count), self.stride * int(count), self.ptr + int(first) * self.stride
        return v

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.shape == (self.height, self.width), (a.shape, self.height, self.width)
        check(self.ctx.lib.schro_hip_upload_2d(
            self.ctx.h, self.ptr, self.stride, a.ctypes.data_as(C.c_void_p), a.strides[0],
            self.width * self.dtype.itemsize, self.height))
        return self

    def download(self):
        out = np.empty((self.height, self.width), self.dtype)
        check(self.ctx.lib.schro_hip_download_2d(
            self.ctx.h, out.ctypes.data_as(C.c_void_p), out.strides[0], self.ptr, self.stride,
            self.width * self.dtype.itemsize, self.height))
        return out

    def upload_async(self, a):
        """Enqueue the copy of `a` (a pinned host array, Context.host_array) on the selected queue."""
        assert a.shape == (self.height, self.width) and a.dtype == self.dtype, (a.shape, a.dtype)
        check(self.ctx.lib.schro_hip_upload_2d_async(
            self.ctx.h, self.ptr, self.stride, a.ctypes.data_as(C.c_void_p), a.strides[0],
            self.width * self.dtype.itemsize, self.height))
        return self

    def download_async(self, out):
        """Enqueue the copy into `out` (a pinned host array) on the selected queue; not waited for."""
        assert out.shape == (self.height, self.width) and out.dtype == self.dtype
        check(self.ctx.lib.schro_hip_download_2d_async(
            self.ctx.h, out.ctypes.data_as(C.c_void_p), out.strides[0], self.ptr, self.stride,
            self.width * self.dtype.itemsize, self.height))
        return out

    def fill(self, byte):
        check(self.ctx.lib.schro_hip_memset(self.ctx.h, self.ptr, byte, self.nbytes))
        return self

    def free(self):
        if self.ptr:
            self.ctx.free(self.ptr)
            self.ptr = None


class HpPlane(DevicePlane):
    """The half-pel (2x upsampled) image of a width x height u8 component: 2*height x
    2*width samples as the four tiled half-pel planes of include/schro_hip.h.
    pair=True: the PAIR image of two such components (the U and V planes of a picture,
    samples interleaved)."""

    def __init__(self, ctx, height, width, pair=False):
        self.ctx = ctx
        self.dtype = np.dtype(np.uint8)
        self.pair = bool(pair)
        self.comp_height, self.comp_width = int(height), int(width)
        self.height, self.width = 2 * self.comp_height, 2 * self.comp_width
        st = C.c_int(0)
        size_of = ctx.lib.schro_hip_upsampled_pair_bytes if pair else ctx.lib.schro_hip_upsampled_bytes
        self.nbytes = size_of(self.comp_width, self.comp_height, C.byref(st))
        self.stride = st.value
        self.ptr = ctx.alloc(self.nbytes)

    def upload(self, a):
        raise SchroHipError("half-pel images are produced by upsample_batch")

    def download(self):
        """Linear (2*height, 2*width) array; a pair image: the two components' arrays."""
        if self.pair:
            u, v = (np.empty((self.height, self.width), np.uint8) for _ in range(2))
            check(self.ctx.lib.schro_hip_upsampled_pair_download(
                self.ctx.h, u.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), u.strides[0], self.ptr,
                self.stride, self.comp_width, self.comp_height))
            return u, v
        out = np.empty((self.height, self.width), np.uint8)
        check(self.ctx.lib.schro_hip_upsampled_download(
            self.ctx.h, out.ctypes.data_as(C.c_void_p), out.strides[0], self.ptr, self.stride,
            self.comp_width, self.comp_height))
        return out


class ArenaPlane(DevicePlane):
    """A height x width plane carved out of a larger device allocation (an arena: all planes of a
    picture batch in ONE block, so that they cross the host boundary as one copy); owns nothing."""

    def __init__(self, arena, offset, height, width, dtype, stride=None):
        self.ctx = arena.ctx
        self.dtype = np.dtype(dtype)
        self.height, self.width = int(height), int(width)
        row = self.width * self.dtype.itemsize
        self.stride = int(stride) if stride else (row + 63) // 64 * 64
        self.nbytes = self.stride * self.height
        assert offset % 256 == 0 and offset + self.nbytes <= arena.nbytes
        self.ptr = arena.ptr + offset

    def free(self):
        self.ptr = None


class Arena:
    """One device block handed out in 256-byte aligned pieces (ArenaPlane)."""

    def __init__(self, ctx, nbytes):
        self.block = DevicePlane(ctx, 1, int(nbytes), np.uint8)
        self.ctx, self.ptr, self.nbytes, self.used = ctx, self.block.ptr, self.block.nbytes, 0

    @staticmethod
    def size_of(shapes_dtypes):
        return sum(((w * np.dtype(d).itemsize + 63) // 64 * 64 * h + 255) // 256 * 256 for (h, w), d in shapes_dtypes)

    def plane(self, height, width, dtype):
        p = ArenaPlane(self, self.used, height, width, dtype)
        self.used += (p.nbytes + 255) // 256 * 256
        return p


class SubPlane:
    """A strided view into a DevicePlane (e.g. the LL band of a coefficient frame in the
    in-place sub-band layout: rows 2^depth apart, stride << depth); owns nothing."""

    def __init__(self, plane, y0, x0, height, width, stride=None):
        self.ctx, self.dtype = plane.ctx, plane.dtype
        self.ptr = plane.ptr + y0 * plane.stride + x0 * plane.dtype.itemsize
        self.height, self.width = int(height), int(width)
        self.stride = int(stride) if stride else plane.stride


class Context:
    """One exec-domain context: device, stream, memory domain."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        self.h = self.lib.schro_hip_context_new(device)
        if not self.h:
            raise SchroHipError("cannot create context on device %d: %s" % (
                device, self.lib.schro_hip_last_error().decode()))
        self.device = device

    def close(self):
        if self.h:
            self.lib.schro_hip_context_free(self.h)
            self.h = None

    def alloc(self, nbytes):
        p = self.lib.schro_hip_domain_alloc(self.h, nbytes)
        if not p:
            raise SchroHipError(self.lib.schro_hip_last_error().decode())
        return p

    def free(self, ptr):
        check(self.lib.schro_hip_domain_free(self.h, ptr))

    def domain_bytes(self):
        return self.lib.schro_hip_domain_bytes(self.h)

    def synchronize(self):
        check(self.lib.schro_hip_synchronize(self.h))

    QUEUE_H2D, QUEUE_D2H = 2, 3

    def queue_synchronize(self, q):
        check(self.lib.schro_hip_queue_synchronize(self.h, q))

    def queue_set_cu_mask(self, q, bits):
        """bits: iterable of 0 / 1 per compute unit (hipExtStreamCreateWithCUMask's bit order)."""
        bits = list(bits)
        words = (len(bits) + 31) // 32
        arr = (C.c_uint32 * words)()
        for n, b in enumerate(bits):
            if b:
                arr[n // 32] |= 1 << (n % 32)
        check(self.lib.schro_hip_queue_set_cu_mask(self.h, q, arr, words))

    def host_array(self, shape, dtype):
        """A numpy array in pinned host memory (schro_hip_host_alloc): what the asynchronous copies
        read and write at full rate.  Freed with the array."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = self.lib.schro_hip_host_alloc(max(n, 1))
        if not p:
            raise SchroHipError(self.lib.schro_hip_last_error().decode())
        buf = (C.c_char * max(n, 1)).from_address(p)
        a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        lib = self.lib
        import weakref
        weakref.finalize(buf, lib.schro_hip_host_free, p)
        return a

    def select_queue(self, q):
        """Calls that follow are enqueued on in-order queue q (0 or 1)."""
        check(self.lib.schro_hip_context_select_queue(self.h, q))

    def queue(self):
        """The queue selected at the moment."""
        return self.lib.schro_hip_context_queue(self.h)

    def queue_mark(self, mark):
        """Record mark (0..15) behind the work enqueued so far on the selected queue."""
        check(self.lib.schro_hip_queue_mark(self.h, mark))

    def queue_wait_mark(self, mark):
        """Later work on the selected queue waits for the latest recording of `mark`."""
        check(self.lib.schro_hip_queue_wait_mark(self.h, mark))

    def queue_mark_synchronize(self, mark):
        """The calling thread waits for the latest recording of `mark` (and for nothing else)."""
        check(self.lib.schro_hip_queue_mark_synchronize(self.h, mark))

    def queue_wait(self, waiter, signaller):
        """Later work on `waiter` starts after everything enqueued so far on `signaller`."""
        check(self.lib.schro_hip_queue_wait(self.h, waiter, signaller))

    def timer_begin(self):
        check(self.lib.schro_hip_timer_begin(self.h))

    def timer_end(self):
        ms = self.lib.schro_hip_timer_end(self.h)
        if ms < 0:
            raise SchroHipError(self.lib.schro_hip_last_error().decode())
        return ms

    KERNEL_CLASSES = ("iiwt_finest", "iiwt_coarse", "upsample", "obmc", "convert", "slices", "dc_predict",
                      "dequant", "quantise", "quantise_dc")

    def profile_enable(self, on=True):
        check(self.lib.schro_hip_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.schro_hip_profile_reset(self.h))

    def profile_read(self):
        """{kernel class: (total_ms, launches)} from the per-launch HIP events."""
        out = {}
        for k, name in enumerate(self.KERNEL_CLASSES):
            ms, n = C.c_double(), C.c_int()
            check(self.lib.schro_hip_profile_read(self.h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def _routes(self, read, names, reset):
        counts = (C.c_longlong * len(names))()
        check(read(self.h, counts, 1 if reset else 0))
        return dict(zip(names, (int(n) for n in counts)))

    OBMC_ROUTES = ("row", "item", "general", "strip")       # SCHRO_HIP_OBMC_ROUTE_* (include/schro_hip.h)

    def obmc_routes(self, reset=False):
        """{route: planes} this context's OBMC calls have handed to the launches of each route (schro_hip_obmc_routes):
        "row" obmc_row*.hip, "item" / "general" obmc.hip's item / per-pixel kernel, "strip" obmc_strip.hip; reset: start
        the counts again from zero after reading them."""
        return self._routes(self.lib.schro_hip_obmc_routes, self.OBMC_ROUTES, reset)

    V210_ROUTES = ("haar3", "level", "two_pass")             # SCHRO_HIP_V210_ROUTE_* (include/schro_hip.h)

    def v210_routes(self, reset=False):
        """{route: pictures} this context's iiwt_pack_v210 calls have handed to each route (schro_hip_v210_routes): "haar3"
        the three-level s32 Haar kernel with the copy-out, "level" the finest level writing v210 (iiwt_v210_kernel), "two_pass"
        the pixel frame in a scratch block and the pack; reset: start the counts again from zero after reading them."""
        return self._routes(self.lib.schro_hip_v210_routes, self.V210_ROUTES, reset)

    PACK8_ROUTES = ("level", "two_pass")                     # SCHRO_HIP_PACK8_ROUTE_* (include/schro_hip.h)

    def pack8_routes(self, reset=False):
        """{route: pictures} this context's iiwt_pack_u8 calls have handed to each route (schro_hip_pack8_routes): "level" the
        finest level writing the packed rows (iiwt_pack8_kernel), "two_pass" the planar picture in a scratch block and the
        pack; reset: start the counts again from zero after reading them."""
        return self._routes(self.lib.schro_hip_pack8_routes, self.PACK8_ROUTES, reset)

    WIDE_ROUTES = ("level", "two_pass")                      # SCHRO_HIP_WIDE_ROUTE_* (include/schro_hip.h)

    def wide_routes(self, reset=False):
        """{route: pictures} this context's iiwt_pack_wide calls have handed to each route (schro_hip_wide_routes): "level" the
        finest level shifting, converting and writing the packed rows (iiwt_wide_kernel), "two_pass" the pixel frame in a
        scratch block, the shift and the pack; reset: start the counts again from zero after reading them."""
        return self._routes(self.lib.schro_hip_wide_routes, self.WIDE_ROUTES, reset)

    UNPACK_ROUTES = ("fused", "two_pass")                    # SCHRO_HIP_UNPACK_ROUTE_* (include/schro_hip.h)

    def unpack_routes(self, reset=False):
        """{route: pictures} this context's unpack_iwt calls have handed to each route (schro_hip_unpack_routes): "fused" the
        forward wavelet's level-0 launch fetching the packed rows itself, "two_pass" the two converts through a scratch block
        and the plane transform; reset: start the counts again from zero after reading them."""
        return self._routes(self.lib.schro_hip_unpack_routes, self.UNPACK_ROUTES, reset)

    def plane(self, height, width, dtype, stride=None):
        return DevicePlane(self, height, width, dtype, stride)

    def hp_plane(self, height, width, pair=False):
        """Half-pel image buffer for a height x width u8 component (upsample_batch's dst); pair: for
        the (U, V) components of a picture together."""
        return HpPlane(self, height, width, pair)

    def upload(self, a, stride=None):
        a = np.ascontiguousarray(a)
        return DevicePlane(self, a.shape[0], a.shape[1], a.dtype, stride).upload(a)

    def upload_bytes(self, a):
        """1-D blob (e.g. a SchroMotionVector array) -> device pointer."""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(1, -1)
        return DevicePlane(self, 1, raw.shape[1], np.uint8).upload(raw)

    # ---- batched plane-level launches (asynchronous on the context stream) ----

    def iiwt_batch(self, pairs, depth, filt, ll=None):
        """pairs: [(src, dst DevicePlane)], all s16 or all s32 -- dst: the residual plane; or, the combine
        form (r04), [(src, out u8 DevicePlane, pred)]: the transform's last step writes the picture
        out = sat_u8 (residual + pred), pred a u8 DevicePlane (the prediction of obmc_batch (prediction_only)) or
        None for a picture without references (+ 128).  ll: per plane, the DevicePlane that holds the LL band of
        this call's coarsest level (the output of an earlier call on the planes' level views, `level_view`)."""
        n = len(pairs)
        arr = (_lib.IwtPlane * n)()
        bpp = pairs[0][0].dtype.itemsize
        for k, t in enumerate(pairs):
            s, d = t[0], t[1]
            assert s.dtype.itemsize == bpp
            if len(t) == 2:
                assert s.dtype == d.dtype
                arr[k] = _lib.IwtPlane(s.ptr, s.stride, d.ptr, d.stride, s.width, s.height, None, 0, 0, 0, 0)
            else:
                pred = t[2]
                assert d.dtype == np.uint8 and (pred is None or (pred.dtype == np.uint8 and (pred.height, pred.width) == (d.height, d.width)))
                arr[k] = _lib.IwtPlane(s.ptr, s.stride, d.ptr, d.stride, s.width, s.height,
                                       pred.ptr if pred is not None else None, pred.stride if pred is not None else 0,
                                       d.width, d.height, 1 if pred is not None else 2)
            if ll is not None:
                q = ll[k]
                assert q.dtype.itemsize == bpp and (q.height, q.width) == (s.height >> depth, s.width >> depth)
                arr[k].ll, arr[k].ll_stride = q.ptr, q.stride
        check(self.lib.schro_hip_iiwt_batch(self.h, arr, n, depth, filt, bpp))

    def iwt_batch(self, pairs, depth, filt):
        """The forward wavelet.  pairs: [(src, dst DevicePlane)], all s16 or all s32 -- src: pixels or residuals, dst: the
        coefficient plane in the in-place sub-band layout (what iiwt_batch takes as its src); sizes may differ."""
        n = len(pairs)
        arr = (_lib.IwtFwdPlane * n)()
        bpp = pairs[0][0].dtype.itemsize
        for k, (s, d) in enumerate(pairs):
            assert s.dtype == d.dtype and s.dtype.itemsize == bpp and (s.height, s.width) == (d.height, d.width)
            arr[k] = _lib.IwtFwdPlane(s.ptr, s.stride, d.ptr, d.stride, s.width, s.height)
        check(self.lib.schro_hip_iwt_batch(self.h, arr, n, depth, filt, bpp))

    def unpack_batch(self, jobs):
        """The encoder-direction schro_frame_convert (schro_hip_unpack_batch).  jobs: (source, dst planes [Y, U, V] of one dtype
        (u8 / s16 / s32), h_shift, v_shift, width, height) per picture; source: (packed plane of bytes, format, src_width,
        src_height) or (planes [Y, U, V] of one dtype, h_shift, v_shift, src_width, src_height).  Pictures of unlike size,
        format and depth mix freely; planes: DevicePlanes or anything with .ptr / .stride / .dtype."""
        n = len(jobs)
        arr = (_lib.UnpackPicture * n)()
        for a, (source, dst, hs, vs, w, h) in zip(arr, jobs):
            if len(source) == 4:
                buf, a.format, a.src_width, a.src_height = source
                a.src[0], a.src_stride[0] = buf.ptr, buf.stride
            else:
                planes, a.src_h_shift, a.src_v_shift, a.src_width, a.src_height = source
                a.src_bpp = np.dtype(planes[0].dtype).itemsize
                for k in range(3):
                    assert np.dtype(planes[k].dtype).itemsize == a.src_bpp
                    a.src[k], a.src_stride[k] = planes[k].ptr, planes[k].stride
            a.dst_bpp = np.dtype(dst[0].dtype).itemsize
            for k in range(3):
                assert np.dtype(dst[k].dtype).itemsize == a.dst_bpp
                a.dst[k], a.dst_stride[k] = dst[k].ptr, dst[k].stride
            a.h_shift, a.v_shift, a.width, a.height = hs, vs, w, h
        check(self.lib.schro_hip_unpack_batch(self.h, arr, n))

    def unpack_iwt_batch(self, jobs, depth, filt):
        """An intra picture from packed bytes to wavelet coefficients (schro_hip_unpack_iwt_batch).  jobs: (packed plane of
        bytes, format, src_width, src_height, picture width, picture height, coefficient planes [Y, U, V] of one dtype (s16 /
        s32), h_shift, v_shift, iwt_width, iwt_height) per picture."""
        n = len(jobs)
        arr = (_lib.UnpackIwtPicture * n)()
        bpp = np.dtype(jobs[0][6][0].dtype).itemsize
        for a, (buf, fmt, sw, sh, w, h, dst, hs, vs, iw, ih) in zip(arr, jobs):
            a.src, a.src_stride, a.format, a.src_width, a.src_height = buf.ptr, buf.stride, fmt, sw, sh
            a.width, a.height, a.h_shift, a.v_shift, a.iwt_width, a.iwt_height = w, h, hs, vs, iw, ih
            for k in range(3):
                assert np.dtype(dst[k].dtype).itemsize == bpp
                a.dst[k], a.dst_stride[k] = dst[k].ptr, dst[k].stride
        check(self.lib.schro_hip_unpack_iwt_batch(self.h, arr, n, depth, filt, bpp))

    def convert_input(self, dest, src):
        """schro_hipframe_convert_input: the encoder-direction schro_frame_convert between two device frames (frames.DeviceFrame):
        src packed or planar, dest planar."""
        check(self.lib.schro_hipframe_convert_input(dest.ptr(), src.ptr()))

    def unpack_iwt_transform(self, iwt_frame, packed, params, picture_width, picture_height):
        """schro_hipframe_unpack_iwt_transform: the packed device frame to the coefficients in iwt_frame (params: a
        _lib.Params, frames.make_params)."""
        check(self.lib.schro_hipframe_unpack_iwt_transform(iwt_frame.ptr(), packed.ptr(), C.byref(params), picture_width, picture_height))

    def downsample_batch(self, jobs):
        """One pyramid level (schro_frame_downsample + schro_frame_mc_edgeextend).  jobs: [(src, dst)] or [(src, dst, ext)],
        u8 DevicePlanes -- dst holds the (h + 1) // 2 x (w + 1) // 2 picture with `ext` samples of apron on every side:
        (h + 1) // 2 + 2 * ext rows of (w + 1) // 2 + 2 * ext samples; sizes may differ."""
        n = len(jobs)
        arr = (_lib.DownsamplePlane * n)()
        for k, t in enumerate(jobs):
            s, d, ext = t[0], t[1], (t[2] if len(t) > 2 else 0)
            assert s.dtype == d.dtype == np.uint8
            assert (d.height, d.width) == ((s.height + 1) // 2 + 2 * ext, (s.width + 1) // 2 + 2 * ext), (d.height, d.width)
            arr[k] = _lib.DownsamplePlane(s.ptr, s.stride, s.width, s.height, d.ptr + ext * d.stride + ext, d.stride, ext)
        check(self.lib.schro_hip_downsample_batch(self.h, arr, n))

    # ---- picture statistics ----

    def plane_sums_batch(self, jobs):
        """schro_hip_plane_sums_batch.  jobs: (a,), (a, b) or (a, b, result) per job -- a: a u8 or s16 plane, b: a u8 plane of
        a's size or None, result: two int64 words of the caller's (.ptr).  Enqueued, not waited for.  Returns the njobs x 2
        int64 DevicePlane [sum of a, sum of (a - b)^2] of the jobs without a result of their own (None when all have one);
        its download () waits."""
        n = len(jobs)
        own = [k for k, t in enumerate(jobs) if len(t) < 3 or t[2] is None]
        res = DevicePlane(self, max(len(own), 1), 2, np.int64, stride=16) if own else None
        full = []
        for k, t in enumerate(jobs):
            r = res.rows_view(own.index(k), 1) if k in own else t[2]
            full.append((t[0], t[1] if len(t) > 1 else None, r))
        check(self.lib.schro_hip_plane_sums_batch(self.h, sums_jobs(full), n))
        return res

    def lowpass2_batch(self, planes):
        """schro_hip_lowpass2_batch: planes filtered IN PLACE.  planes: (plane, h, v) or (plane, h, v, counter) per plane --
        plane u8 or s16, h and v a sigma or the four coefficients, counter a uint32 word of the caller's (.ptr) that the call
        ADDS its out-of-range samples to.  Returns the nplanes' x 1 uint32 DevicePlane (cleared) of the planes without a
        counter of their own, None when all have one."""
        n = len(planes)
        own = [k for k, t in enumerate(planes) if len(t) < 4 or t[3] is None]
        cnt = DevicePlane(self, max(len(own), 1), 1, np.uint32, stride=4).fill(0) if own else None
        full = [(t[0], t[1], t[2], cnt.rows_view(own.index(k), 1) if k in own else t[3]) for k, t in enumerate(planes)]
        check(self.lib.schro_hip_lowpass2_batch(self.h, lowpass2_planes(full), n))
        return cnt

    def ssim_batch(self, pictures):
        """schro_hip_ssim_batch.  pictures: (a, b), (a, b, map) or (a, b, map, scratch, result) per picture -- a, b u8 planes
        of one size; map: True for a float64 DevicePlane of the per-pixel values, a plane of the caller's, or None; scratch
        (a span of ssim_scratch_bytes bytes) and result (SSIM_RESULT_DTYPE, 32 bytes) the caller's or allocated here.
        Enqueued, not waited for.  Returns per picture (result, map, scratch): download result and view it as
        SSIM_RESULT_DTYPE (ssim_result); keep scratch until the queue has been waited for."""
        full, out = [], []
        for t in pictures:
            a, b = t[0], t[1]
            m = t[2] if len(t) > 2 else None
            if m is True:
                m = DevicePlane(self, a.height, a.width, np.float64)
            scratch = t[3] if len(t) > 3 and t[3] is not None else DevicePlane(self, 1, max(ssim_scratch_bytes(a.width, a.height), 16), np.uint8)
            result = t[4] if len(t) > 4 and t[4] is not None else DevicePlane(self, 1, SSIM_RESULT_DTYPE.itemsize, np.uint8)
            full.append((a, b, m, scratch, result))
            out.append((result, m, scratch))
        check(self.lib.schro_hip_ssim_batch(self.h, ssim_pictures(full), len(full)))
        return out

    @staticmethod
    def ssim_result(result):
        """(sum, [out_of_range x 5]) of one picture's result plane (waits: a download)."""
        r = result.download().reshape(-1).view(SSIM_RESULT_DTYPE)[0]
        return float(r["sum"]), [int(v) for v in r["out_of_range"]]

    def average_luma(self, frame):
        """schro_hipframe_calculate_average_luma of a device frame (frames.DeviceFrame / PlaneFrame): the reference's value,
        its int accumulator's wrap included."""
        out = C.c_double()
        check(self.lib.schro_hipframe_calculate_average_luma(frame.ptr(), C.byref(out)))
        return out.value

    def mean_squared_error(self, a, b):
        """schro_hipframe_mean_squared_error of two u8 device frames: [mse Y, U, V]."""
        out = (C.c_double * 3)()
        check(self.lib.schro_hipframe_mean_squared_error(a.ptr(), b.ptr(), out))
        return [float(v) for v in out]

    def ssim(self, a, b):
        """schro_hipframe_ssim of two u8 device frames: mssim of the luma planes."""
        out = C.c_double()
        check(self.lib.schro_hipframe_ssim(a.ptr(), b.ptr(), C.byref(out)))
        return out.value

    def filter_lowpass2(self, frame, sigma):
        """schro_hipframe_filter_lowpass2: the u8 or s16 device frame low-passed in place (the pre-filter `filtering = 2`)."""
        check(self.lib.schro_hipframe_filter_lowpass2(frame.ptr(), float(sigma)))

    def scene_change_score(self, frame1, frame2, average_luma):
        """schro_engine_get_scene_change_score_hip: frame1, frame2 the coarsest pyramid levels of a picture and its
        predecessor, average_luma that of frame1 (Context.average_luma)."""
        out = C.c_double()
        check(self.lib.schro_engine_get_scene_change_score_hip(frame1.ptr(), frame2.ptr(), float(average_luma), C.byref(out)))
        return out.value

    def metric_scan_batch(self, pictures, tables=True):
        """The SAD scans of schro_metric_scan_do_scan + schro_metric_scan_get_min.  pictures: [(frame, ref, extension,
        scans)] -- frame, ref: u8 DevicePlanes of one size, scans: a SCAN_DTYPE array.  Returns [(results, metrics)] per
        picture, DevicePlanes to download: results nscans x 4 int32 (dx, dy, metric, 0), metrics nscans x 42 * 42 uint32
        (entry i * scan_height + j of each scan; None without `tables`)."""
        n = len(pictures)
        arr = (_lib.MetricScanPicture * n)()
        out, keep = [], []
        for k, (f, r, ext, scans) in enumerate(pictures):
            assert f.dtype == r.dtype == np.uint8 and (f.height, f.width) == (r.height, r.width)
            scans = np.ascontiguousarray(scans, dtype=SCAN_DTYPE)
            keep.append(scans)
            res = DevicePlane(self, max(len(scans), 1), 4, np.int32, stride=16)
            met = DevicePlane(self, max(len(scans), 1), LIMIT_METRIC_SCAN ** 2, np.uint32, stride=4 * LIMIT_METRIC_SCAN ** 2) if tables else None
            arr[k] = _lib.MetricScanPicture(f.ptr, f.stride, r.ptr, r.stride, f.width, f.height, ext,
                                            scans.ctypes.data_as(C.POINTER(_lib.MetricScan)), len(scans), res.ptr,
                                            met.ptr if met is not None else None)
            out.append((res, met))
        try:
            check(self.lib.schro_hip_metric_scan_batch(self.h, arr, n))
        except SchroHipError:
            for res, met in out:
                res.free()
                if met is not None:
                    met.free()
            raise
        return out

    def rough_scan_nohint(self, frame, ref, params, shift, distance, ref_index, extension=0):
        """schro_rough_me_heirarchical_scan_nohint over two u8 luma DevicePlanes that are already at pyramid level `shift`
        (schro_rough_me_heirarchical_scan_nohint_hip on frames made of them).  params: a dict with x_num_blocks,
        y_num_blocks, xbsep_luma, ybsep_luma (or a _lib.Params).  Returns the MV_DTYPE array, complete."""
        from . import frames
        if not isinstance(params, _lib.Params):
            params = frames.make_params(**{k: params[k] for k in ("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma")})
        fa, fb = frames.PlaneFrame(self, [frame] * 3, extension), frames.PlaneFrame(self, [ref] * 3, extension)
        mvs = np.zeros(params.x_num_blocks * params.y_num_blocks, MV_DTYPE)
        check(self.lib.schro_rough_me_heirarchical_scan_nohint_hip(fa.ptr(), fb.ptr(), C.byref(params), shift, distance, ref_index,
                                                                   mvs.ctypes.data_as(C.c_void_p)))
        return mvs

    def motion_field(self, params):
        """A device motion field: x_num_blocks * y_num_blocks SchroMotionVector records (one row of a DevicePlane)."""
        nbx, nby = _block_geometry(params)[:2]
        return DevicePlane(self, 1, nbx * nby * MV_DTYPE.itemsize, np.uint8, stride=nbx * nby * MV_DTYPE.itemsize)

    @staticmethod
    def download_field(field):
        """The MV_DTYPE records of a device motion field: rme->motion_fields[shift] as it is."""
        return field.download().reshape(-1).view(MV_DTYPE).copy()

    def rough_hint_batch(self, pictures):
        """One hint level of the rough search per picture (schro_rough_me_heirarchical_scan_hint), one launch:
        pictures as rough_hint_pictures takes them.  Every record of each `field` is written; enqueued, not waited for."""
        check(self.lib.schro_hip_rough_hint_batch(self.h, rough_hint_pictures(pictures), len(pictures)))

    def rough_me_batch(self, chains, nohint_distance=12, hint_distance=4):
        """schro_rough_me_heirarchical_scan per chain, one launch: chains as rough_chains takes them -- the nohint level at
        n_levels, then the hint levels down to 1, the fields staying on the device.  Enqueued, not waited for."""
        arr, keep = rough_chains(chains)
        check(self.lib.schro_hip_rough_me_batch(self.h, arr, len(chains), nohint_distance, hint_distance))

    def rough_scan_hint(self, frame, ref, params, shift, distance, ref_index, hint_mvs, extension=0):
        """schro_rough_me_heirarchical_scan_hint_hip over two u8 luma DevicePlanes at pyramid level `shift`; hint_mvs: the
        MV_DTYPE array of level shift + 1.  Returns the MV_DTYPE array of level `shift`, complete."""
        from . import frames
        if not isinstance(params, _lib.Params):
            params = frames.make_params(**dict(zip(("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"), _block_geometry(params))))
        fa, fb = frames.PlaneFrame(self, [frame] * 3, extension), frames.PlaneFrame(self, [ref] * 3, extension)
        hint = np.ascontiguousarray(hint_mvs, dtype=MV_DTYPE)
        assert hint.size == params.x_num_blocks * params.y_num_blocks
        mvs = np.zeros(hint.size, MV_DTYPE)
        check(self.lib.schro_rough_me_heirarchical_scan_hint_hip(fa.ptr(), fb.ptr(), C.byref(params), shift, distance, ref_index,
                                                                 hint.ctypes.data_as(C.c_void_p), mvs.ctypes.data_as(C.c_void_p)))
        return mvs

    def rough_scan(self, frames_by_level, refs_by_level, params, ref_index, extension=0):
        """schro_rough_me_heirarchical_scan_hip: frames_by_level[k], refs_by_level[k] are the u8 luma DevicePlanes at
        pyramid level k for k = 1 .. n_levels (entry 0, the full picture, is not read and may be None).  Returns the list
        of MV_DTYPE arrays by level (entry 0: None), complete."""
        from . import frames
        if not isinstance(params, _lib.Params):
            params = frames.make_params(**dict(zip(("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"), _block_geometry(params))))
        n = len(frames_by_level) - 1
        assert len(refs_by_level) == n + 1
        fa = [None] + [frames.PlaneFrame(self, [p] * 3, extension) for p in frames_by_level[1:]]
        fb = [None] + [frames.PlaneFrame(self, [p] * 3, extension) for p in refs_by_level[1:]]
        pa, pb = (C.POINTER(_lib.Frame) * (n + 1))(), (C.POINTER(_lib.Frame) * (n + 1))()
        out = [None] + [np.zeros(params.x_num_blocks * params.y_num_blocks, MV_DTYPE) for _ in range(n)]
        fields = (C.c_void_p * (n + 1))()
        for k in range(1, n + 1):
            pa[k], pb[k], fields[k] = C.pointer(fa[k].c), C.pointer(fb[k].c), out[k].ctypes.data
        check(self.lib.schro_rough_me_heirarchical_scan_hip(pa, pb, C.byref(params), n, ref_index, fields))
        return out

    def hbm_level_batch(self, levels):
        """One level of the hierarchical block matching per entry (schro_hierarchical_bm_scan_hint), one launch: levels as
        hbm_levels takes them.  Every record of each `field` is written; enqueued, not waited for."""
        check(self.lib.schro_hip_hbm_level_batch(self.h, hbm_levels(levels), len(levels)))

    def hbm_batch(self, chains, with_level0=True):
        """schro_hbm_scan per chain and, with_level0, the level-0 call behind it, one launch: chains as hbm_chains takes
        them, the fields staying on the device.  Enqueued, not waited for."""
        arr, keep = hbm_chains(chains)
        check(self.lib.schro_hip_hbm_batch(self.h, arr, len(chains), int(bool(with_level0))))

    def _hbm_params(self, params):
        from . import frames
        if isinstance(params, _lib.Params):
            return params
        return frames.make_params(**dict(zip(("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"), _block_geometry(params))))

    def hbm_scan_hint(self, frame, ref, params, shift, h_range, ref_index, hint_mvs=None, extension=0, h_shift=0, v_shift=0):
        """schro_hierarchical_bm_scan_hint_hip over the (Y, U, V) u8 DevicePlanes of two frames at pyramid level `shift`,
        each plane with `extension` samples of apron on every side; hint_mvs: the MV_DTYPE array of level shift + 1 or
        None.  Returns the MV_DTYPE array of level `shift`, complete."""
        from . import frames
        params = self._hbm_params(params)
        fa = frames.PlaneFrame(self, frame, extension, h_shift, v_shift)
        fb = frames.PlaneFrame(self, ref, extension, h_shift, v_shift)
        n = params.x_num_blocks * params.y_num_blocks
        hint = None
        if hint_mvs is not None:
            hint = np.ascontiguousarray(hint_mvs, dtype=MV_DTYPE)
            assert hint.size == n
        mvs = np.zeros(n, MV_DTYPE)
        check(self.lib.schro_hierarchical_bm_scan_hint_hip(fa.ptr(), fb.ptr(), C.byref(params), shift, h_range, ref_index,
                                                           hint.ctypes.data_as(C.c_void_p) if hint is not None else None,
                                                           mvs.ctypes.data_as(C.c_void_p)))
        return mvs

    def hbm_scan(self, frames_by_level, refs_by_level, params, ref_index, with_level0=True, extension=0, h_shift=0, v_shift=0):
        """schro_hbm_scan_hip: frames_by_level[k], refs_by_level[k] are the (Y, U, V) u8 DevicePlanes at pyramid level k for
        k = 0 .. n_levels, each with `extension` samples of apron (entry 0 is not read and may be None without
        with_level0).  Returns the list of MV_DTYPE arrays by level (entry 0: None without with_level0), complete."""
        from . import frames
        params = self._hbm_params(params)
        n = len(frames_by_level) - 1
        assert len(refs_by_level) == n + 1
        first = 0 if with_level0 else 1
        fa = [frames.PlaneFrame(self, p, extension, h_shift, v_shift) if k >= first else None for k, p in enumerate(frames_by_level)]
        fb = [frames.PlaneFrame(self, p, extension, h_shift, v_shift) if k >= first else None for k, p in enumerate(refs_by_level)]
        pa, pb = (C.POINTER(_lib.Frame) * (n + 1))(), (C.POINTER(_lib.Frame) * (n + 1))()
        out = [np.zeros(params.x_num_blocks * params.y_num_blocks, MV_DTYPE) if k >= first else None for k in range(n + 1)]
        fields = (C.c_void_p * (n + 1))()
        for k in range(first, n + 1):
            pa[k], pb[k], fields[k] = C.pointer(fa[k].c), C.pointer(fb[k].c), out[k].ctypes.data
        check(self.lib.schro_hbm_scan_hip(pa, pb, C.byref(params), n, ref_index, int(bool(with_level0)), fields))
        return out

    def subpel_error_batch(self, chains, mvprec, tables):
        """The errors of precision pass `mvprec` of the sub-pel refinement, one launch over the blocks of all chains: chains
        as subpel_chains takes them; tables[c] -- device memory (anything with ptr) for 8 * x_num_blocks * y_num_blocks
        int32, written whole; the fields are read.  Enqueued, not waited for."""
        check(self.lib.schro_hip_subpel_error_batch(self.h, subpel_chains(chains), len(chains), mvprec, _subpel_tables(tables)))

    def subpel_choose_batch(self, chains, mvprec, tables):
        """The choice of precision pass `mvprec` from the given tables: each chain's `field` is doubled and refined in place,
        one workgroup per chain.  Enqueued, not waited for."""
        check(self.lib.schro_hip_subpel_choose_batch(self.h, subpel_chains(chains), len(chains), mvprec, _subpel_tables(tables)))

    def subpel_batch(self, chains):
        """schro_encoder_motion_predict_subpel_deep per chain: field <- src_field, then mv_precision x (errors, choice) with
        tables from the context's scratch.  Enqueued, not waited for."""
        check(self.lib.schro_hip_subpel_batch(self.h, subpel_chains(chains), len(chains)))

    def subpel_deep(self, src, ref_upframes, params, lam, fields, extension=32):
        """schro_encoder_motion_predict_subpel_deep_hip: src -- the u8 luma DevicePlane of the picture with `extension`
        samples of apron on every side; ref_upframes -- one upsampled frames.DeviceFrame per reference; params -- a dict
        (or _lib.Params) with the block geometry and mv_precision; fields -- the MV_DTYPE level-0 field of each reference.
        Returns the refined MV_DTYPE arrays, complete."""
        from . import frames
        if not isinstance(params, _lib.Params):
            params = frames.make_params(mv_precision=params["mv_precision"],
                                        **dict(zip(("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"), _block_geometry(params))))
        n = len(ref_upframes)
        assert len(fields) == n
        params.num_refs = n
        fa = frames.PlaneFrame(self, [src] * 3, extension)
        out = [np.ascontiguousarray(f, dtype=MV_DTYPE).copy() for f in fields]
        ups, ptrs = (C.POINTER(_lib.Frame) * n)(), (C.c_void_p * n)()
        for k in range(n):
            assert out[k].size == params.x_num_blocks * params.y_num_blocks
            ups[k], ptrs[k] = ref_upframes[k].ptr(), out[k].ctypes.data
        check(self.lib.schro_encoder_motion_predict_subpel_deep_hip(fa.ptr(), ups, C.byref(params), float(lam), ptrs))
        return out

    def split2_metric_batch(self, pictures, tables):
        """What the split-2 mode decision reads from the pictures, one launch over the blocks of all of them: pictures as
        split2_pictures takes them; tables[c] -- device memory (anything with ptr) for SPLIT2_TABLE_INTS int32 per block,
        written whole.  Enqueued, not waited for."""
        check(self.lib.schro_hip_split2_metric_batch(self.h, split2_pictures(pictures), len(pictures), _subpel_tables(tables)))

    def split2_choose_batch(self, pictures, tables):
        """The choice from the given tables and the sub-pel fields: motion and superblocks are written, one workgroup per
        picture.  Enqueued, not waited for."""
        check(self.lib.schro_hip_split2_choose_batch(self.h, split2_pictures(pictures), len(pictures), _subpel_tables(tables)))

    def split2_batch(self, pictures):
        """schro_do_split2 for every superblock of every picture: both launches, tables from the context's scratch.
        Enqueued, not waited for."""
        check(self.lib.schro_hip_split2_batch(self.h, split2_pictures(pictures), len(pictures)))

    def mode_decision_split2(self, src_planes, ref_upframes, params, lam, fields, extension=32, h_shift=1, v_shift=1):
        """schro_mode_decision_split2_hip: src_planes -- the u8 Y, U, V DevicePlanes of the picture, each with `extension`
        samples of apron on every side; ref_upframes -- one upsampled frames.DeviceFrame per reference; params -- a dict
        with the block geometry and mv_precision; fields -- the MV_DTYPE sub-pel field of each reference.  Returns (motion
        as MV_DTYPE, the superblocks as SB_DTYPE), complete."""
        from . import frames
        nbx, nby, xb, yb = _block_geometry(params)
        P = frames.make_params(mv_precision=params["mv_precision"], x_num_blocks=nbx, y_num_blocks=nby, xbsep_luma=xb, ybsep_luma=yb)
        n = len(ref_upframes)
        assert len(fields) == n
        P.num_refs = n
        fa = frames.PlaneFrame(self, src_planes, extension, h_shift, v_shift)
        keep = [np.ascontiguousarray(f, dtype=MV_DTYPE) for f in fields]
        ups, ptrs = (C.POINTER(_lib.Frame) * n)(), (C.c_void_p * n)()
        for k in range(n):
            assert keep[k].size == nbx * nby
            ups[k], ptrs[k] = ref_upframes[k].ptr(), keep[k].ctypes.data
        motion, sb = np.zeros(nbx * nby, MV_DTYPE), np.zeros(nbx * nby // 16, SB_DTYPE)
        check(self.lib.schro_mode_decision_split2_hip(fa.ptr(), ups, C.byref(P), float(lam), ptrs, motion.ctypes.data, sb.ctypes.data))
        return motion, sb

    def mode_metric_batch(self, pictures, tables):
        """What the whole mode decision reads from the pictures without a decision: pictures as mode_pictures takes them;
        tables[2 c] -- device memory for SPLIT2_TABLE_INTS int32 per block, tables[2 c + 1] -- for MODE_TABLE_INTS int32 per
        superblock, both written whole.  Two launches over all pictures.  Enqueued, not waited for."""
        check(self.lib.schro_hip_mode_metric_batch(self.h, mode_pictures(pictures), len(pictures), _subpel_tables(tables)))

    def mode_choose_batch(self, pictures, tables):
        """The walk from the given tables: motion, superblocks, trials and stats are written, one workgroup per picture.
        Enqueued, not waited for."""
        check(self.lib.schro_hip_mode_choose_batch(self.h, mode_pictures(pictures), len(pictures), _subpel_tables(tables)))

    def mode_decision_batch(self, pictures):
        """schro_mode_decision for every picture: the metric launches and the walk, tables from the context's scratch.
        Enqueued, not waited for."""
        check(self.lib.schro_hip_mode_decision_batch(self.h, mode_pictures(pictures), len(pictures)))

    def mode_decision(self, src_planes, ref_upframes, params, lam, fields, level1, level2, extension=32, h_shift=1, v_shift=1):
        """schro_mode_decision_hip: as mode_decision_split2, and level1, level2 -- the MV_DTYPE level-1 and level-2 field of
        the block matching per reference.  Returns (motion as MV_DTYPE, the superblocks as SB_DTYPE, the trials as
        (superblocks, 4) MODE_TRIAL_DTYPE, the three statistics), complete."""
        from . import frames
        nbx, nby, xb, yb = _block_geometry(params)
        P = frames.make_params(mv_precision=params["mv_precision"], x_num_blocks=nbx, y_num_blocks=nby, xbsep_luma=xb, ybsep_luma=yb)
        n = len(ref_upframes)
        assert len(fields) == n and len(level1) == n and len(level2) == n
        P.num_refs = n
        fa = frames.PlaneFrame(self, src_planes, extension, h_shift, v_shift)
        keep = [np.ascontiguousarray(f, dtype=MV_DTYPE) for f in fields]
        levels = [np.ascontiguousarray(f[k], dtype=MV_DTYPE) for k in range(n) for f in (level1, level2)]
        ups, ptrs, lptrs = (C.POINTER(_lib.Frame) * n)(), (C.c_void_p * n)(), (C.c_void_p * (2 * n))()
        for k in range(n):
            assert keep[k].size == nbx * nby and levels[2 * k].size == nbx * nby and levels[2 * k + 1].size == nbx * nby
            ups[k], ptrs[k] = ref_upframes[k].ptr(), keep[k].ctypes.data
            lptrs[2 * k], lptrs[2 * k + 1] = levels[2 * k].ctypes.data, levels[2 * k + 1].ctypes.data
        motion, sb = np.zeros(nbx * nby, MV_DTYPE), np.zeros(nbx * nby // 16, SB_DTYPE)
        trials, stats = np.zeros((nbx * nby // 16, 4), MODE_TRIAL_DTYPE), np.zeros(3, np.float64)
        check(self.lib.schro_mode_decision_hip(fa.ptr(), ups, C.byref(P), float(lam), ptrs, lptrs, motion.ctypes.data, sb.ctypes.data,
                                               trials.ctypes.data, stats.ctypes.data_as(C.POINTER(C.c_double))))
        return motion, sb, trials, stats

    def pack_u8_batch(self, jobs):
        """jobs: (planes [Y, U, V] DevicePlanes, h_shift, v_shift, dst DevicePlane of 4-byte
        groups, width, height, format) per picture."""
        n = len(jobs)
        arr = (_lib.PackPlane * n)()
        for a, (planes, hs, vs, dst, w, h, fmt) in zip(arr, jobs):
            for k in range(3):
                a.src[k] = planes[k].ptr
                a.src_stride[k] = planes[k].stride
            a.src_width, a.src_height = planes[0].width, planes[0].height
            a.src_h_shift, a.src_v_shift = hs, vs
            a.dst, a.dst_stride = dst.ptr, dst.stride
            a.width, a.height, a.format = w, h, fmt
        check(self.lib.schro_hip_pack_u8_batch(self.h, arr, n))

    def pack_v210_batch(self, jobs):
        """jobs: (planes [Y, U, V] DevicePlanes of one dtype (u8 / s16 / s32), h_shift, v_shift,
        dst DevicePlane of bytes, width, height) per picture."""
        n = len(jobs)
        arr = (_lib.PackPlane * n)()
        bpp = jobs[0][0][0].dtype.itemsize
        for a, (planes, hs, vs, dst, w, h) in zip(arr, jobs):
            assert planes[0].dtype.itemsize == bpp
            for k in range(3):
                a.src[k] = planes[k].ptr
                a.src_stride[k] = planes[k].stride
            a.src_width, a.src_height = planes[0].width, planes[0].height
            a.src_h_shift, a.src_v_shift = hs, vs
            a.dst, a.dst_stride = dst.ptr, dst.stride
            a.width, a.height, a.format = w, h, FORMAT_V210
        check(self.lib.schro_hip_pack_v210_batch(self.h, arr, n, bpp))

    @staticmethod
    def _iiwt_pack_picture(a, bpp, planes, hs, vs, dst, w, h):
        """The fields the pictures of the three iiwt_pack_*_batch calls have in common."""
        for k in range(3):
            assert planes[k].dtype.itemsize == bpp
            a.src[k] = planes[k].ptr
            a.src_stride[k] = planes[k].stride
        a.width, a.height = planes[0].width, planes[0].height
        a.h_shift, a.v_shift = hs, vs
        a.dst, a.dst_stride = dst.ptr, dst.stride
        a.out_width, a.out_height = w, h

    def iiwt_pack_v210_batch(self, jobs, depth, filt):
        """r05: the inverse wavelet and the v210 copy-out in one call.  jobs: (coefficient planes [Y, U, V] DevicePlanes of one
        dtype, h_shift, v_shift, dst DevicePlane of bytes, picture width, picture height) per picture."""
        n = len(jobs)
        arr = (_lib.IwtPackPicture * n)()
        bpp = jobs[0][0][0].dtype.itemsize
        for a, job in zip(arr, jobs):
            self._iiwt_pack_picture(a, bpp, *job)
        check(self.lib.schro_hip_iiwt_pack_v210_batch(self.h, arr, n, depth, filt, bpp))

    def iiwt_pack_u8_batch(self, jobs, depth, filt):
        """The inverse wavelet, the add of the prediction (or of 128) and the YUYV / UYVY / AYUV copy-out in one call.  jobs:
        (coefficient planes [Y, U, V] of one dtype, h_shift, v_shift, predictions [Y, U, V] u8 planes or None (a picture
        without references), dst plane of bytes, picture width, picture height, format) per picture; planes: DevicePlanes
        or SubPlanes."""
        n = len(jobs)
        arr = (_lib.IwtPack8Picture * n)()
        bpp = jobs[0][0][0].dtype.itemsize
        for a, (planes, hs, vs, preds, dst, w, h, fmt) in zip(arr, jobs):
            self._iiwt_pack_picture(a, bpp, planes, hs, vs, dst, w, h)
            for k in range(3 if preds is not None else 0):
                assert preds[k].dtype == np.uint8
                a.pred[k] = preds[k].ptr
                a.pred_stride[k] = preds[k].stride
            a.format = fmt
        check(self.lib.schro_hip_iiwt_pack_u8_batch(self.h, arr, n, depth, filt, bpp))

    def iiwt_pack_wide_batch(self, jobs, depth, filt):
        """The inverse wavelet, schro_frame_shift_right and the v216 / ARGB / AY64 copy-out in one call.  jobs: (coefficient
        planes [Y, U, V] of one dtype (s16 / s32), h_shift, v_shift, dst plane of bytes, picture width, picture height, format,
        shift) per picture; planes: DevicePlanes or SubPlanes."""
        n = len(jobs)
        arr = (_lib.IwtPackWidePicture * n)()
        bpp = jobs[0][0][0].dtype.itemsize
        for a, (*common, fmt, shift) in zip(arr, jobs):
            self._iiwt_pack_picture(a, bpp, *common)
            a.format, a.shift = fmt, shift
        check(self.lib.schro_hip_iiwt_pack_wide_batch(self.h, arr, n, depth, filt, bpp))

    def pack_wide_batch(self, jobs):
        """jobs: (planes [Y, U, V] DevicePlanes of one dtype, h_shift, v_shift, dst DevicePlane of
        bytes, width, height, format (FORMAT_V216 / FORMAT_ARGB / FORMAT_AY64)) per picture."""
        n = len(jobs)
        arr = (_lib.PackPlane * n)()
        bpp = jobs[0][0][0].dtype.itemsize
        for a, (planes, hs, vs, dst, w, h, fmt) in zip(arr, jobs):
            assert planes[0].dtype.itemsize == bpp
            for k in range(3):
                a.src[k] = planes[k].ptr
                a.src_stride[k] = planes[k].stride
            a.src_width, a.src_height = planes[0].width, planes[0].height
            a.src_h_shift, a.src_v_shift = hs, vs
            a.dst, a.dst_stride = dst.ptr, dst.stride
            a.width, a.height, a.format = w, h, fmt
        check(self.lib.schro_hip_pack_wide_batch(self.h, arr, n, bpp))

    def shift_right_batch(self, planes, shift):
        """schro_frame_shift_right on DevicePlanes (s16 / s32), in place."""
        n = len(planes)
        arr = (_lib.DcPlane * n)()
        for a, p in zip(arr, planes):
            a.data, a.stride, a.width, a.height = p.ptr, p.stride, p.width, p.height
        check(self.lib.schro_hip_shift_right_batch(self.h, arr, n, planes[0].dtype.itemsize, shift))

    @staticmethod
    def lowdelay_params(P):
        """dict with the SchroParams members of the slice decode -> the ABI struct."""
        lp = _lib.LowDelayParams()
        for name in ("transform_depth", "iwt_luma_width", "iwt_luma_height", "iwt_chroma_width",
                     "iwt_chroma_height", "n_horiz_slices", "n_vert_slices", "slice_bytes_num",
                     "slice_bytes_denom"):
            setattr(lp, name, int(P[name]))
        for k, q in enumerate(P["quant_matrix"]):
            lp.quant_matrix[k] = int(q)
        return lp

    def lowdelay_arith(self, P, bpp):
        r = self.lib.schro_hip_lowdelay_arith(C.byref(self.lowdelay_params(P)), bpp)
        check(min(r, 0))
        return r

    def lowdelay_batch(self, pictures, P):
        """pictures: (slice bytes on the device (upload_bytes), [Y, U, V] coefficient
        DevicePlanes) per picture; P: the parameter dict.  Mirrors
        schro_decoder_decode_lowdelay_transform_data."""
        n = len(pictures)
        arr = (_lib.LowDelayPicture * n)()
        bpp = pictures[0][1][0].dtype.itemsize
        for a, (sl, planes) in zip(arr, pictures):
            a.slices, a.slices_bytes = sl.ptr, sl.width
            for k in range(3):
                assert planes[k].dtype.itemsize == bpp
                a.comp[k], a.stride[k] = planes[k].ptr, planes[k].stride
        check(self.lib.schro_hip_lowdelay_batch(self.h, arr, n, C.byref(self.lowdelay_params(P)), bpp))

    def lowdelay_encode_batch(self, pictures, P, bpp=None):
        """schro_hip_lowdelay_encode_batch.  pictures: per picture the [Y, U, V] coefficient DevicePlanes (s16; not
        written) or (planes, slices, base_index, overruns) with caller-owned device buffers (u8 DevicePlanes of one row,
        overruns 4 bytes); P: the parameter dict.  Mirrors schro_encoder_encode_lowdelay_transform_data.  Where the
        buffers are the call's own, waits and returns per picture (bytes uint8 array, base indices uint8 array, number of
        over-run slices); with caller-owned buffers the call is asynchronous and returns None."""
        n = len(pictures)
        arr = (_lib.LowDelayEncodePicture * n)()
        nbytes = (int(P["slice_bytes_num"]) * int(P["n_horiz_slices"]) * int(P["n_vert_slices"])
                  // max(int(P["slice_bytes_denom"]), 1))
        nslices = int(P["n_horiz_slices"]) * int(P["n_vert_slices"])
        own = []
        for a, pic in zip(arr, pictures):
            if isinstance(pic, tuple) and len(pic) == 4:
                planes, sl, idx, ovr = pic
                sb = sl.width
            else:
                sb = nbytes
                planes = pic
                sl = DevicePlane(self, 1, max(nbytes, 1), np.uint8)
                idx = DevicePlane(self, 1, max(nslices, 1), np.uint8)
                ovr = DevicePlane(self, 1, 1, np.uint32)
                own.append((sl, idx, ovr))
            for k in range(3):
                a.comp[k], a.stride[k] = planes[k].ptr, planes[k].stride
            a.slices, a.slices_bytes = sl.ptr, sb
            a.base_index, a.overruns = idx.ptr, ovr.ptr
        if bpp is None:
            first = pictures[0][0] if isinstance(pictures[0], tuple) and len(pictures[0]) == 4 else pictures[0]
            bpp = first[0].dtype.itemsize
        try:
            check(self.lib.schro_hip_lowdelay_encode_batch(self.h, arr, n, C.byref(self.lowdelay_params(P)), bpp))
            if not own:
                return None
            return [(sl.download()[0, :nbytes].copy(), idx.download()[0, :nslices].copy(), int(ovr.download()[0, 0]))
                    for sl, idx, ovr in own]
        finally:
            for bufs in own:
                for b in bufs:
                    b.free()

    def encode_lowdelay(self, iwt_frame, P):
        """schro_hip_encode_lowdelay_transform_data on a device frame (frames.DeviceFrame / PlaneFrame, s16): (bytes,
        base indices, number of over-run slices), the first what the reference appends to frame->pack."""
        nslices = int(P["n_horiz_slices"]) * int(P["n_vert_slices"])
        nbytes = int(P["slice_bytes_num"]) * nslices // int(P["slice_bytes_denom"])
        data, idx = np.zeros(max(nbytes, 1), np.uint8), np.zeros(nslices, np.uint8)
        ovr = C.c_int(0)
        check(self.lib.schro_hip_encode_lowdelay_transform_data(iwt_frame.ptr(), data.ctypes.data, nbytes,
                                                                C.byref(self.lowdelay_params(P)), idx.ctypes.data, C.byref(ovr)))
        return data[:nbytes], idx, int(ovr.value)

    def noarith_encode_batch(self, pictures, capacity=None):
        """schro_hip_noarith_encode_batch.  pictures: per picture (planes, tables, depth, horiz_codeblocks, vert_codeblocks,
        codeblock_mode_index) -- as noarith_pictures takes them -- or the same followed by (out, capacity, result) with
        caller-owned device buffers (a u8 DevicePlane, its capacity in bytes, a DevicePlane of a SchroHipNoarithResult).
        Mirrors schro_encoder_encode_transform_data for is_noarith without its quantiser call.  Where the buffers are the
        call's own -- `capacity` bytes each, or noarith_encode_bound -- waits and returns per picture (bytes uint8 array
        cut at the capacity, noarith_result dict); with caller-owned buffers the call is asynchronous and returns None."""
        return self._noarith_encode(pictures, capacity, lambda arr, n, bpp: self.lib.schro_hip_noarith_encode_batch(self.h, arr, n, bpp))

    def noarith_encode_chosen_batch(self, pictures, chosen, clamped, capacity=None):
        """schro_hip_noarith_encode_chosen_batch: noarith_encode_batch with the quant indices taken from device memory.
        The records' quant_index holds their sub-band; chosen: per picture the device address of its 3 x 19 int32 chosen
        indices (SchroHipQuantChoice.quant_index: anything with ptr, or an address); clamped: a device word the caller has
        cleared (anything with ptr, or an address), added to for every sub-band whose index lay outside 0 .. 60."""
        addr = lambda m: getattr(m, "ptr", m)
        ptrs = (C.c_void_p * len(chosen))(*[addr(c) for c in chosen])
        assert len(chosen) == len(pictures)
        return self._noarith_encode(pictures, capacity, lambda arr, n, bpp: self.lib.schro_hip_noarith_encode_chosen_batch(
            self.h, arr, ptrs, n, bpp, addr(clamped)))

    def _noarith_encode(self, pictures, capacity, call):
        bpp = pictures[0][0][0].dtype.itemsize
        own, full = [], []
        words = C.sizeof(_lib.NoarithResult) // 4
        for pic in pictures:
            if len(pic) == 9:
                full.append(tuple(pic))
                continue
            planes, tables, depth, hc, vc, mode = pic
            cap = capacity if capacity is not None else noarith_encode_bound([(p.width, p.height) for p in planes], depth, hc, vc, bpp)
            out = DevicePlane(self, 1, max(cap, 1), np.uint8)
            res = DevicePlane(self, 1, words, np.uint32)
            own.append((out, res, cap))
            full.append((planes, tables, depth, hc, vc, mode, out, cap, res))
        try:
            arr, keep = noarith_pictures(full)
            check(call(arr, len(full), bpp))
            if not own:
                return None
            got = []
            for out, res, cap in own:
                r = noarith_result(res.download())
                got.append((out.download()[0, :min(cap, r["bytes"])].copy(), r))
            return got
        finally:
            for out, res, cap in own:
                out.free()
                res.free()

    def noarith_decode_batch(self, pictures):
        """schro_hip_noarith_decode_batch.  pictures: per picture (data, coeffs, quant, depth, horiz_codeblocks,
        vert_codeblocks, codeblock_mode_index, is_intra, compat_quant_offset) -- data: the HOST bytes (uint8 array or bytes);
        coeffs, quant as noarith_decode_pictures takes them -- or the twelve entries of noarith_decode_pictures with
        caller-owned device buffers.  Mirrors schro_decoder_parse_transform_data + schro_decoder_decode_transform_data for
        is_noarith.  Where the bytes and the result are the call's own, waits and returns a noarith_decode_result dict per
        picture; with caller-owned buffers the call is asynchronous and returns None."""
        bpp = np.dtype(pictures[0][3][0].dtype if len(pictures[0]) == 12 else pictures[0][1][0].dtype).itemsize
        own, full = [], []
        words = C.sizeof(_lib.NoarithDecodeResult) // 4
        try:
            for pic in pictures:
                if len(pic) == 12:
                    full.append(tuple(pic))
                    continue
                data, coeffs, quant, depth, hc, vc, mode, is_intra, compat = pic
                raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
                dev = DevicePlane(self, 1, max(raw.size, 1), np.uint8)
                res = DevicePlane(self, 1, words, np.uint32)
                own.append((dev, res))
                if raw.size:
                    dev.upload(raw.reshape(1, -1))
                full.append((dev, int(raw.size), None, coeffs, quant, depth, hc, vc, mode, is_intra, compat, res))
            check(self.lib.schro_hip_noarith_decode_batch(self.h, noarith_decode_pictures(full), len(full), bpp))
            if not own:
                return None
            return [noarith_decode_result(res.download()) for dev, res in own]
        finally:
            for dev, res in own:
                dev.free()
                res.free()

    def decode_transform_data_noarith(self, transform_frame, data, params, compat_quant_offset):
        """schro_hipframe_decode_transform_data_noarith on a device frame (frames.DeviceFrame, s16 / s32): the HOST bytes go
        up, the frame is filled as schro_hipframe_dequantise leaves it.  Returns (noarith_decode_result dict, the compat
        state after the picture, status) -- status 0, or SCHRO_HIP_EINVAL (-1) with result["error"] set when a header holds
        a quant index above 60 (the frame is untouched); any other status raises."""
        raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
        compat = C.c_int(int(bool(compat_quant_offset)))
        res = _lib.NoarithDecodeResult()
        rc = self.lib.schro_hipframe_decode_transform_data_noarith(transform_frame.ptr(), raw.ctypes.data if raw.size else None, raw.size,
                                                                   C.byref(params), C.byref(compat), C.byref(res))
        if rc != 0 and not (rc == -1 and res.error):
            check(rc)
        return noarith_decode_result(res), int(compat.value), rc

    def arith_decode_batch(self, pictures):
        """schro_hip_arith_decode_batch: Context.noarith_decode_batch for arithmetic-coded transform data (the form a default
        encoder writes), with the same two shapes of `pictures`.  Where the bytes and the result are the call's own, waits
        and returns an arith_decode_result dict per picture; with caller-owned buffers the call is asynchronous and returns
        None.  The LL bands of an intra picture are not DC-predicted (dc_predict_batch)."""
        bpp = np.dtype(pictures[0][3][0].dtype if len(pictures[0]) == 12 else pictures[0][1][0].dtype).itemsize
        own, full = [], []
        words = C.sizeof(_lib.ArithDecodeResult) // 4
        try:
            for pic in pictures:
                if len(pic) == 12:
                    full.append(tuple(pic))
                    continue
                data, coeffs, quant, depth, hc, vc, mode, is_intra, compat = pic
                raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
                dev = DevicePlane(self, 1, max(raw.size, 1), np.uint8)
                res = DevicePlane(self, 1, words, np.uint32)
                own.append((dev, res))
                if raw.size:
                    dev.upload(raw.reshape(1, -1))
                full.append((dev, int(raw.size), None, coeffs, quant, depth, hc, vc, mode, is_intra, compat, res))
            check(self.lib.schro_hip_arith_decode_batch(self.h, arith_decode_pictures(full), len(full), bpp))
            if not own:
                return None
            return [arith_decode_result(res.download()) for dev, res in own]
        finally:
            for dev, res in own:
                dev.free()
                res.free()

    def decode_transform_data_arith(self, transform_frame, data, params, compat_quant_offset):
        """schro_hipframe_decode_transform_data_arith on a device frame (frames.DeviceFrame, s16 / s32): the HOST bytes go
        up, the frame is filled as schro_hipframe_dequantise leaves it.  Returns (arith_decode_result dict, the compat
        state after the picture, status) -- status 0, or SCHRO_HIP_EINVAL (-1) with result["error"] set when a header holds
        a quant index above 60 (the frame is untouched); any other status raises (params.is_noarith, params.is_lowdelay)."""
        raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
        compat = C.c_int(int(bool(compat_quant_offset)))
        res = _lib.ArithDecodeResult()
        rc = self.lib.schro_hipframe_decode_transform_data_arith(transform_frame.ptr(), raw.ctypes.data if raw.size else None, raw.size,
                                                                 C.byref(params), C.byref(compat), C.byref(res))
        if rc != 0 and not (rc == -1 and res.error):
            check(rc)
        return arith_decode_result(res), int(compat.value), rc

    def motion_encode_batch(self, pictures, capacity=None):
        """schro_hip_motion_encode_batch.  pictures: per picture (motion, x_num_blocks, y_num_blocks, num_refs,
        have_global_motion) -- motion: the device field (anything with ptr) -- or the same followed by (out, capacity,
        result) with caller-owned device buffers.  Mirrors schroencoder.c:2505-2515 for is_noarith.  Where the buffers
        are the call's own -- `capacity` bytes each, or motion_encode_bound -- waits and returns per picture (bytes uint8
        array cut at the capacity, motion_encode_result dict); with caller-owned buffers the call is asynchronous and
        returns None."""
        own, full = [], []
        words = C.sizeof(_lib.MotionEncodeResult) // 4
        try:
            for pic in pictures:
                if len(pic) == 8:
                    full.append(tuple(pic))
                    continue
                motion, nbx, nby, num_refs, hg = pic
                cap = capacity if capacity is not None else motion_encode_bound(nbx, nby, num_refs, hg)
                out = DevicePlane(self, 1, max(cap, 1), np.uint8)
                res = DevicePlane(self, 1, words, np.uint32)
                own.append((out, res, cap))
                full.append((motion, nbx, nby, num_refs, hg, out, cap, res))
            check(self.lib.schro_hip_motion_encode_batch(self.h, motion_encode_pictures(full), len(full)))
            if not own:
                return None
            got = []
            for out, res, cap in own:
                r = motion_encode_result(res.download())
                got.append((out.download()[0, :min(cap, r["bytes"])].copy(), r))
            return got
        finally:
            for out, res, cap in own:
                out.free()
                res.free()

    def encode_motion_data_noarith(self, field, params, capacity):
        """schro_hip_encode_motion_data_noarith on a HOST field (MV_DTYPE records, params.x_num_blocks x y_num_blocks):
        (bytes uint8 array, bytes the picture takes, section_bytes (9), motion_encode_result dict, status) -- status 0, or
        SCHRO_HIP_ENOMEM (-3) when the picture takes more than `capacity`; any other status raises."""
        field = np.ascontiguousarray(field)
        motion = _lib.Motion()
        motion.motion_vectors = field.ctypes.data
        data = np.zeros(max(capacity, 1), np.uint8)
        nbytes = C.c_size_t(0)
        sec = (C.c_int * _lib.MOTION_SECTIONS)()
        res = _lib.MotionEncodeResult()
        rc = self.lib.schro_hip_encode_motion_data_noarith(self.h, C.byref(motion), C.byref(params), data.ctypes.data, capacity,
                                                           C.byref(nbytes), sec, C.byref(res))
        if rc not in (0, -3) or (rc == -3 and nbytes.value <= capacity):
            check(rc)
        words = np.frombuffer(bytes(res), np.uint32)
        return data[:min(capacity, nbytes.value)], int(nbytes.value), list(sec), motion_encode_result(words), rc

    def motion_decode_batch(self, pictures):
        """schro_hip_motion_decode_batch.  pictures: per picture (data, x_num_blocks, y_num_blocks, num_refs,
        have_global_motion) -- data: the HOST bytes -- or the nine members of motion_decode_pictures with caller-owned device
        buffers.  Mirrors schrodecoder.c:2531-2814 for is_noarith.  Where the buffers are the call's own it waits and
        returns per picture (field of MV_DTYPE records, motion_decode_result dict); with caller-owned buffers the call is
        asynchronous and returns None."""
        own, full = [], []
        words = C.sizeof(_lib.MotionDecodeResult) // 4
        try:
            for pic in pictures:
                if len(pic) == 9:
                    full.append(tuple(pic))
                    continue
                data, nbx, nby, num_refs, hg = pic
                raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
                dev = DevicePlane(self, 1, max(raw.size, 1), np.uint8)
                field = DevicePlane(self, 1, nbx * nby * MV_DTYPE.itemsize, np.uint8)
                res = DevicePlane(self, 1, words, np.uint32)
                own.append((dev, field, res))
                if raw.size:
                    dev.upload(raw.reshape(1, -1))
                full.append((dev, raw.size, None, nbx, nby, num_refs, hg, field, res))
            check(self.lib.schro_hip_motion_decode_batch(self.h, motion_decode_pictures(full), len(full)))
            if not own:
                return None
            return [(field.download().reshape(-1).view(MV_DTYPE).copy(), motion_decode_result(res.download())) for dev, field, res in own]
        finally:
            for bufs in own:
                for b in bufs:
                    b.free()

    def decode_motion_data_noarith(self, data, params):
        """schro_hip_decode_motion_data_noarith: the HOST bytes to the HOST field of params.x_num_blocks x y_num_blocks
        MV_DTYPE records and the motion_decode_result dict."""
        raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
        field = np.full(params.x_num_blocks * params.y_num_blocks, 0xff, np.uint8).repeat(MV_DTYPE.itemsize).view(MV_DTYPE)
        motion = _lib.Motion()
        motion.motion_vectors = field.ctypes.data
        res = _lib.MotionDecodeResult()
        check(self.lib.schro_hip_decode_motion_data_noarith(self.h, raw.ctypes.data if raw.size else None, raw.size, C.byref(params),
                                                            C.byref(motion), C.byref(res)))
        return field, motion_decode_result(np.frombuffer(bytes(res), np.uint32))

    def motion_arith_decode_batch(self, pictures):
        """schro_hip_motion_arith_decode_batch, as motion_decode_batch: per picture (data, x_num_blocks, y_num_blocks,
        num_refs, have_global_motion) -- data: the HOST bytes -- or the nine members of motion_arith_decode_pictures with
        caller-owned device buffers.  Mirrors schrodecoder.c:2531-2814 for !is_noarith.  Where the buffers are the call's
        own it waits and returns per picture (field of MV_DTYPE records, motion_arith_decode_result dict); with
        caller-owned buffers the call is asynchronous and returns None."""
        own, full = [], []
        words = C.sizeof(_lib.MotionArithDecodeResult) // 4
        try:
            for pic in pictures:
                if len(pic) == 9:
                    full.append(tuple(pic))
                    continue
                data, nbx, nby, num_refs, hg = pic
                raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
                dev = DevicePlane(self, 1, max(raw.size, 1), np.uint8)
                field = DevicePlane(self, 1, nbx * nby * MV_DTYPE.itemsize, np.uint8)
                res = DevicePlane(self, 1, words, np.uint32)
                own.append((dev, field, res))
                if raw.size:
                    dev.upload(raw.reshape(1, -1))
                full.append((dev, raw.size, None, nbx, nby, num_refs, hg, field, res))
            check(self.lib.schro_hip_motion_arith_decode_batch(self.h, motion_arith_decode_pictures(full), len(full)))
            if not own:
                return None
            return [(field.download().reshape(-1).view(MV_DTYPE).copy(), motion_arith_decode_result(res.download()))
                    for dev, field, res in own]
        finally:
            for bufs in own:
                for b in bufs:
                    b.free()

    def decode_motion_data_arith(self, data, params):
        """schro_hip_decode_motion_data_arith: the HOST bytes to the HOST field of params.x_num_blocks x y_num_blocks
        MV_DTYPE records and the motion_arith_decode_result dict."""
        raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
        field = np.full(params.x_num_blocks * params.y_num_blocks, 0xff, np.uint8).repeat(MV_DTYPE.itemsize).view(MV_DTYPE)
        motion = _lib.Motion()
        motion.motion_vectors = field.ctypes.data
        res = _lib.MotionArithDecodeResult()
        check(self.lib.schro_hip_decode_motion_data_arith(self.h, raw.ctypes.data if raw.size else None, raw.size, C.byref(params),
                                                          C.byref(motion), C.byref(res)))
        return field, motion_arith_decode_result(np.frombuffer(bytes(res), np.uint32))

    def encode_transform_data_noarith(self, quant_frame, params, quant_indices, capacity):
        """schro_hip_encode_transform_data_noarith on a device frame (frames.DeviceFrame, s16 / s32) that
        schro_hipframe_quantise filled: (bytes uint8 array, bytes the picture takes, subband_bits (3 x 19), false_zero
        (codeblocks, sub-bands), status) -- status 0, or SCHRO_HIP_ENOMEM (-3) when the picture takes more than
        `capacity`; any other status raises.  quant_indices: per component the quant index of every record."""
        idx = [np.ascontiguousarray(q, np.int32) for q in quant_indices]
        qi = (C.POINTER(C.c_int) * 3)(*[q.ctypes.data_as(C.POINTER(C.c_int)) for q in idx])
        data = np.zeros(max(capacity, 1), np.uint8)
        nbytes = C.c_size_t(0)
        bits = ((C.c_int * _lib.NOARITH_MAX_SUBBANDS) * 3)()
        fz = (C.c_int * 2)()
        rc = self.lib.schro_hip_encode_transform_data_noarith(quant_frame.ptr(), C.byref(params), qi, data.ctypes.data, capacity,
                                                              C.byref(nbytes), bits, fz)
        if rc not in (0, -3) or (rc == -3 and nbytes.value <= capacity):
            check(rc)
        return (data[:min(capacity, nbytes.value)], int(nbytes.value), np.array([list(b) for b in bits], np.int64),
                (int(fz[0]), int(fz[1])), rc)

    @staticmethod
    def codeblock_table(cbs):
        """The C table (SchroHipCodeblock array) of a list of (dst_offset, dst_stride, width, height,
        src_offset, src_bytes, quant_index): build it once per picture, not per call."""
        tab = (_lib.Codeblock * len(cbs))()
        for t, cb in zip(tab, cbs):
            (t.dst_offset, t.dst_stride, t.width, t.height, t.src_offset, t.src_bytes, t.quant_index) = cb
        return tab

    def codeblock_layout(self, width, height, depth, horiz_codeblocks, vert_codeblocks, stride, itemsize):
        """schro_hip_codeblock_layout: the geometry of every codeblock record of a component (C table)."""
        hc = (C.c_int * (depth + 1))(*horiz_codeblocks)
        vc = (C.c_int * (depth + 1))(*vert_codeblocks)
        n = self.lib.schro_hip_codeblock_layout(width, height, depth, hc, vc, stride, itemsize, None, 0)
        if n < 0:
            raise SchroHipError(self.lib.schro_hip_last_error().decode())
        tab = (_lib.Codeblock * n)()
        check(min(0, self.lib.schro_hip_codeblock_layout(width, height, depth, hc, vc, stride, itemsize, tab, n)))
        return tab

    def dequant_batch(self, jobs, arith=0):
        """jobs: (dst DevicePlane (s16 / s32), values device blob (DevicePlane of bytes, or an object
        with .ptr) or None, codeblocks -- a C table from codeblock_table / codeblock_layout or a list
        of (dst_offset, dst_stride, width, height, src_offset, src_bytes, quant_index) --,
        is_intra) per component."""
        n = len(jobs)
        arr = (_lib.DequantPlane * n)()
        keep = []
        for a, (dst, values, cbs, intra) in zip(arr, jobs):
            tab = cbs if isinstance(cbs, C.Array) else self.codeblock_table(cbs)
            keep.append(tab)
            a.dst, a.values = dst.ptr, values.ptr if values is not None else None
            a.codeblocks, a.ncodeblocks, a.is_intra = tab, len(cbs), 1 if intra else 0
        check(self.lib.schro_hip_dequant_batch(self.h, arr, n, jobs[0][0].dtype.itemsize, arith))

    def _dequant_planes(self, jobs):
        n = len(jobs)
        arr = (_lib.DequantPlane * n)()
        keep = []
        for a, (dst, values, cbs, intra) in zip(arr, jobs):
            tab = cbs if isinstance(cbs, C.Array) else self.codeblock_table(cbs)
            keep.append(tab)
            a.dst, a.values = dst.ptr, values.ptr if values is not None else None
            a.codeblocks, a.ncodeblocks, a.is_intra = tab, len(cbs), 1 if intra else 0
        return arr, keep

    def dequant_plan(self, jobs, arith=0):
        """schro_hip_dequant_plan_new over `jobs` (as dequant_batch takes them): the geometry of their codeblock
        records, resident on the device.  plan.run(jobs) dequantises a batch with the same geometry."""
        return DequantPlan(self, jobs, arith)

    def dc_predict_batch(self, planes):
        """In-place DC prediction of LL bands given as DevicePlanes (s16 / s32)."""
        n = len(planes)
        arr = (_lib.DcPlane * n)()
        for a, p in zip(arr, planes):
            a.data, a.stride, a.width, a.height = p.ptr, p.stride, p.width, p.height
        check(self.lib.schro_hip_dc_predict_batch(self.h, arr, n, planes[0].dtype.itemsize))

    def convert_u8_batch(self, pairs):
        n = len(pairs)
        arr = (_lib.ConvertPlane * n)()
        bpp = pairs[0][0].dtype.itemsize
        for k, (s, d) in enumerate(pairs):
            arr[k] = _lib.ConvertPlane(s.ptr, s.stride, d.ptr, d.stride, d.width, d.height)
        check(self.lib.schro_hip_convert_u8_batch(self.h, arr, n, bpp))

    def add_batch(self, pairs):
        """pairs: [(dst s16 DevicePlane, src s16 | u8 DevicePlane)]: dst += src over their common size
        (schro_frame_add / schro_gpuframe_add on planes)."""
        n = len(pairs)
        arr = (_lib.ConvertPlane * n)()
        for k, (d, s) in enumerate(pairs):
            assert d.dtype == np.int16 and s.dtype.itemsize == pairs[0][1].dtype.itemsize
            arr[k] = _lib.ConvertPlane(s.ptr, s.stride, d.ptr, d.stride, min(d.width, s.width), min(d.height, s.height))
        check(self.lib.schro_hip_add_batch(self.h, arr, n, pairs[0][1].dtype.itemsize))

    def subtract_batch(self, pairs):
        """pairs: [(dst s16 DevicePlane, src s16 | u8 DevicePlane)]: dst -= src over their common size
        (schro_frame_subtract on planes)."""
        n = len(pairs)
        arr = (_lib.ConvertPlane * n)()
        for k, (d, s) in enumerate(pairs):
            assert d.dtype == np.int16 and s.dtype == pairs[0][1].dtype and s.dtype in (np.int16, np.uint8)
            arr[k] = _lib.ConvertPlane(s.ptr, s.stride, d.ptr, d.stride, min(d.width, s.width), min(d.height, s.height))
        check(self.lib.schro_hip_subtract_batch(self.h, arr, n, 1 if pairs[0][1].dtype == np.uint8 else 0))

    def quantise_batch(self, jobs):
        """schro_hip_quantise_batch.  jobs: per component (coeffs DevicePlane (s16 / s32), quant DevicePlane of the same
        layout, codeblocks -- a C table or a list of (dst_offset, dst_stride, width, height, src_offset, src_bytes,
        quant_index) --, is_intra[, (dc_predict_first, dc_width, dc_height)]).  The coefficient planes receive the
        reconstruction, the quant planes the quantised values.  Returns one DevicePlane per component holding its
        SchroHipCodeblockSummary entries (download (): an (ncodeblocks, 2) uint32 array of nonzero, max_abs)."""
        return self._quantise(jobs, lambda arr, n, bpp: self.lib.schro_hip_quantise_batch(self.h, arr, n, bpp))

    def _quantise(self, jobs, call):
        n = len(jobs)
        arr = (_lib.QuantPlane * n)()
        keep, summaries = [], []
        for a, job in zip(arr, jobs):
            coeffs, quant, cbs, intra = job[:4]
            dc = job[4] if len(job) > 4 and job[4] else (0, 0, 0)
            tab = cbs if isinstance(cbs, C.Array) else self.codeblock_table(cbs)
            keep.append(tab)
            assert quant.dtype == coeffs.dtype and quant.stride == coeffs.stride and quant.height >= coeffs.height
            summ = DevicePlane(self, len(tab), 2, np.uint32, stride=8)
            summaries.append(summ)
            a.coeffs, a.quant, a.bytes = coeffs.ptr, quant.ptr, coeffs.stride * coeffs.height
            a.codeblocks, a.ncodeblocks, a.is_intra = tab, len(tab), 1 if intra else 0
            a.dc_predict_first, a.dc_width, a.dc_height = dc
            a.summary = summ.ptr
        check(call(arr, n, jobs[0][0].dtype.itemsize))
        return summaries

    def quantise_chosen_batch(self, jobs, chosen, clamped):
        """schro_hip_quantise_chosen_batch: quantise_batch with the quant indices taken from device memory.  jobs: as
        quantise_batch takes them, the records' quant_index holding their sub-band; chosen: per job the device address of
        its component's row of 19 int32 chosen indices (SchroHipQuantChoice.quant_index[component]: anything with ptr, or
        an address); clamped: a device word the caller has cleared, added to for every record whose index lay outside
        0 .. 60.  Enqueued, not waited for.  Returns the summaries as quantise_batch does."""
        addr = lambda m: getattr(m, "ptr", m)
        assert len(chosen) == len(jobs)
        ptrs = (C.c_void_p * len(chosen))(*[addr(c) for c in chosen])
        return self._quantise(jobs, lambda arr, n, bpp: self.lib.schro_hip_quantise_chosen_batch(self.h, arr, ptrs, n, bpp, addr(clamped)))

    def histogram_planes(self, jobs):
        """The C table of a schro_hip_histogram_batch call and its device counts.  jobs: per component (coeffs DevicePlane
        (s16 / s32), bands -- a list of (offset, stride, width, height, skip, dc_predict): bytes, bytes, samples, samples).
        Returns (SchroHipHistogramPlane array, per component a view of its (nbands, 105) uint32 counts, the block): ONE
        DevicePlane holds the counts of all components (the call clears counts that lie one behind the other with one
        memset) and the band tables the array points to; the caller keeps it while the array is used and frees it."""
        arr = (_lib.HistogramPlane * len(jobs))()
        size = C.sizeof(_lib.HistogramCounts)
        block = DevicePlane(self, sum(len(bands) for _, bands in jobs), _lib.HISTOGRAM_BINS + 1, np.uint32, stride=size)
        block.tables, counts, first = [], [], 0
        for a, (coeffs, bands) in zip(arr, jobs):
            tab = (_lib.HistogramBand * len(bands))(*[_lib.HistogramBand(*(int(v) for v in b)) for b in bands])
            block.tables.append(tab)
            cnt = block.rows_view(first, len(bands))
            counts.append(cnt)
            first += len(bands)
            a.coeffs, a.bytes, a.bands, a.nbands, a.counts = coeffs.ptr, coeffs.stride * coeffs.height, tab, len(bands), cnt.ptr
        return arr, counts, block

    def histogram_batch(self, jobs):
        """schro_hip_histogram_batch over `jobs` (see histogram_planes): the raw counts of every band, before the scale by
        skip -- per component an (nbands, 105) uint32 array, 104 bins and the overflow word.  Waits for the result."""
        arr, counts, block = self.histogram_planes(jobs)
        try:
            check(self.lib.schro_hip_histogram_batch(self.h, arr, len(jobs), jobs[0][0].dtype.itemsize))
            return [c.download() for c in counts]
        finally:
            block.free()

    def subband_histograms(self, iwt_frame, params):
        """schro_hipframe_subband_histograms on a device frame (frames.DeviceFrame / PlaneFrame): (n, bins, overflow) --
        an int array of 3 * (1 + 3 * depth) entries, a float64 array of as many rows of 104 bins, a uint32 array -- what
        schro_encoder_generate_subband_histograms leaves in frame->subband_hists, component-major."""
        nh = 3 * (1 + 3 * params.transform_depth)
        hists = (_lib.Histogram * nh)()
        ovf = (C.c_uint32 * nh)()
        check(self.lib.schro_hipframe_subband_histograms(iwt_frame.ptr(), C.byref(params), hists, ovf))
        return (np.array([h.n for h in hists], np.int64), np.array([list(h.bins) for h in hists], np.float64).reshape(nh, -1),
                np.array(list(ovf), np.uint32))

    def quant_choose_tables(self, error, onebits=None, zerobits=None):
        """schro_hip_quant_choose_tables: the encoder's error table (60 x 104 doubles) and, for pictures that are not
        noarith, its one-bits / zero-bits tables, into the context's device memory.  Replaces earlier ones."""
        tabs = [None if t is None else np.ascontiguousarray(t, np.float64) for t in (error, onebits, zerobits)]
        for t in tabs:
            assert t is None or t.shape == (_lib.QUANT_CHOOSE_INDICES, _lib.HISTOGRAM_BINS), t.shape
        dp = C.POINTER(C.c_double)
        check(self.lib.schro_hip_quant_choose_tables(self.h, *[None if t is None else t.ctypes.data_as(dp) for t in tabs]))

    def quant_choose_batch(self, pictures, estimates=False):
        """schro_hip_quant_choose_batch over `pictures` (quant_choose_pictures' dicts; `result` may be left out: one
        DevicePlane of QUANT_CHOICE_DTYPE rows is made for the call).  Enqueued, not waited for.  Returns the results'
        DevicePlane (download ().view (QUANT_CHOICE_DTYPE): a row per picture; row p's quant_index starts
        QUANT_CHOICE_DTYPE.fields["quant_index"][1] bytes into it) and, with estimates=True, a DevicePlane of
        2 x len (pictures) rows of 3 x 19 x 60 doubles: est_entropy, then est_error, per picture."""
        n = len(pictures)
        size = QUANT_CHOICE_DTYPE.itemsize
        res = DevicePlane(self, n, size, np.uint8, stride=size)
        est = DevicePlane(self, 2 * n, 3 * _lib.QUANT_CHOOSE_BANDS * _lib.QUANT_CHOOSE_INDICES, np.float64) if estimates else None
        full = []
        for k, p in enumerate(pictures):
            p = dict(p)
            p.setdefault("result", res.ptr + k * size)
            if est is not None:
                p["est_entropy"], p["est_error"] = est.ptr + 2 * k * est.stride, est.ptr + (2 * k + 1) * est.stride
            full.append(p)
        check(self.lib.schro_hip_quant_choose_batch(self.h, quant_choose_pictures(full), n))
        return (res, est) if estimates else res

    def choose_quantisers(self, iwt_frame, params, is_noarith, engine, target, weight, ratio, scales):
        """schro_encoder_choose_quantisers_hip on a device frame (frames.DeviceFrame / PlaneFrame): the histograms, the
        choice, and the SchroHipQuantChoice on the host -- a QUANT_CHOICE_DTYPE record.  Waits.  weight: per sub-band;
        ratio: [3][sub-bands]; scales: (sub-band 0, chroma, diagonal)."""
        s = _lib.QuantChooseSettings()
        s.is_noarith, s.engine, s.target = int(is_noarith), int(engine), float(target)
        for i, w in enumerate(list(weight)[:_lib.QUANT_CHOOSE_BANDS]):
            s.subband_weight[i] = float(w)
        for c in range(3):
            for i, r in enumerate(list(ratio[c])[:_lib.QUANT_CHOOSE_BANDS]):
                s.context_ratio[c][i] = float(r)
        s.subband0_lambda_scale, s.chroma_lambda_scale, s.diagonal_lambda_scale = (float(v) for v in scales)
        out = np.zeros(1, QUANT_CHOICE_DTYPE)
        check(self.lib.schro_encoder_choose_quantisers_hip(iwt_frame.ptr(), C.byref(params), C.byref(s), out.ctypes.data_as(C.c_void_p)))
        return out[0]

    def upsample_batch(self, pairs):
        """pairs: [(src u8 plane h x w, dst HpPlane)] or [((src U, src V), dst pair HpPlane)]."""
        n = len(pairs)
        arr = (_lib.UpsamplePlane * n)()
        for k, (s, d) in enumerate(pairs):
            sv = None
            if isinstance(s, (tuple, list)):
                s, sv = s
                assert getattr(d, "pair", False) and (sv.height, sv.width) == (s.height, s.width)
            else:
                assert not getattr(d, "pair", False)
            assert d.height == 2 * s.height and d.width == 2 * s.width
            arr[k] = _lib.UpsamplePlane(s.ptr, s.stride, d.ptr, d.stride, s.width, s.height,
                                        sv.ptr if sv is not None else None, sv.stride if sv is not None else 0)
        check(self.lib.schro_hip_upsample_batch(self.h, arr, n))

    def obmc_batch(self, planes):
        n = len(planes)
        arr = (_lib.ObmcPlane * n)(*planes)
        check(self.lib.schro_hip_obmc_batch(self.h, arr, n))


def obmc_plane(mvs, params, component, ref1, ref2, residual, out, prediction_only=False):
    """Fill a SchroHipObmcPlane.  params: dict with the SchroParams motion fields
    plus chroma_h_shift / chroma_v_shift; mvs: DevicePlane holding the records.
    prediction_only (residual None): `out` receives the prediction for iiwt_batch's combine form."""
    p = _lib.ObmcPlane()
    p.mvs = mvs.ptr
    for name in ("x_num_blocks", "y_num_blocks", "xblen_luma", "yblen_luma", "xbsep_luma",
                 "ybsep_luma", "mv_precision", "picture_weight_bits", "picture_weight_1",
                 "picture_weight_2", "chroma_h_shift", "chroma_v_shift"):
        setattr(p, name, int(params[name]))
    p.component = component
    p.ref1, p.ref1_stride = ref1.ptr, ref1.stride
    if ref2 is not None:
        p.ref2, p.ref2_stride = ref2.ptr, ref2.stride
    if residual is not None:        # None: nothing to add (a zero_residual picture)
        p.residual, p.residual_stride = residual.ptr, residual.stride
        p.residual_bpp = residual.dtype.itemsize
    p.out, p.out_stride = out.ptr, out.stride
    p.width, p.height = out.width, out.height
    # (prediction_only 2, r06: `out` is an s16 plane that receives the prediction - 128)
    p.prediction_only = int(prediction_only)
    p.ref_pair = 1 if getattr(ref1, "pair", False) else 0      # (U, V) pair images (HpPlane (pair=True))
    assert ref2 is None or bool(getattr(ref2, "pair", False)) == bool(p.ref_pair)
    return p


class DequantPlan:
    def __init__(self, ctx, jobs, arith=0):
        self.ctx = ctx
        arr, keep = ctx._dequant_planes(jobs)
        self.h = ctx.lib.schro_hip_dequant_plan_new(ctx.h, arr, len(jobs), jobs[0][0].dtype.itemsize, arith)
        if not self.h:
            raise SchroHipError(ctx.lib.schro_hip_last_error().decode())

    def planes(self, jobs):
        """The C array of a batch (dst, values, C table, is_intra per component): build it once per frame pool."""
        return self.ctx._dequant_planes(jobs)

    def run(self, jobs=None, planes=None):
        if planes is None:
            planes = self.planes(jobs)
        check(self.ctx.lib.schro_hip_dequant_plan_run(self.h, planes[0], len(planes[0])))

    def free(self):
        if self.h:
            self.ctx.lib.schro_hip_dequant_plan_free(self.h)
            self.h = None


class Scheduler:
    """schro_hip_scheduler_*: one exec-domain thread and context per device; pictures follow
    their references (include/schro_hip.h).  func(ctx, device_index) is the picture's pixel
    path; ctx is a Context of that device (None on virtual devices)."""

    def __init__(self, n_devices=0, virtual=False, devices=None):
        self.lib = _lib.load()
        if devices is not None:         # an explicit list; a device may repeat (two contexts on one GPU)
            arr = (C.c_int * len(devices))(*devices)
            self.h = self.lib.schro_hip_scheduler_new_on(arr, len(devices))
        else:
            self.h = (self.lib.schro_hip_scheduler_new_virtual if virtual
                      else self.lib.schro_hip_scheduler_new)(n_devices)
        if not self.h:
            raise SchroHipError(self.lib.schro_hip_last_error().decode())
        self.n_devices = self.lib.schro_hip_scheduler_n_devices(self.h)
        self.contexts = []
        for k in range(self.n_devices):
            hctx = self.lib.schro_hip_scheduler_context(self.h, k)
            c = None
            if hctx:
                c = Context.__new__(Context)
                c.lib, c.h, c.device = self.lib, hctx, k
            self.contexts.append(c)
        self._keep = []

    def submit(self, number, refs, is_ref, func):
        """Returns (device index, foreign reference or -1)."""
        def thunk(hctx, index, priv):
            try:
                return int(func(self.contexts[index], index) or 0)
            except Exception:       # an exception must not unwind into the C thread
                import traceback
                traceback.print_exc()
                return -99
        cb = _lib.PICTURE_FUNC(thunk)
        self._keep.append(cb)
        arr = (C.c_int * max(len(refs), 1))(*refs)
        foreign = C.c_int(-1)
        dev = self.lib.schro_hip_scheduler_submit(self.h, number, arr, len(refs), 1 if is_ref else 0, cb, None,
                                                  C.byref(foreign))
        if dev < 0:
            raise SchroHipError(self.lib.schro_hip_last_error().decode())
        return dev, foreign.value

    def retire(self, number):
        check(self.lib.schro_hip_scheduler_retire(self.h, number))

    def publish_reference(self, device_index, frame_ptr):
        """Called by a reference picture's function: the device frame (SchroHipFrame pointer; any
        non-zero token on virtual devices) its dependents read."""
        check(self.lib.schro_hip_scheduler_publish_reference(self.h, device_index, frame_ptr))

    def reference_frame(self, device_index, number):
        """Called by a picture's function: the frame of its reference `number` on this device."""
        return self.lib.schro_hip_scheduler_reference_frame(self.h, device_index, number)

    def moves(self):
        return self.lib.schro_hip_scheduler_moves(self.h)

    def skipped(self):
        """Pictures that did not run because a reference of theirs had failed (or had been skipped)."""
        return self.lib.schro_hip_scheduler_skipped(self.h)

    def refs_in_flight_max(self):
        """Most reference pictures of one device whose device work was still running at once."""
        return self.lib.schro_hip_scheduler_refs_in_flight_max(self.h)

    def wait(self):
        r = self.lib.schro_hip_scheduler_wait(self.h)
        self._keep = []
        return r

    def close(self):
        if self.h:
            self.lib.schro_hip_scheduler_free(self.h)
            self.h = None
