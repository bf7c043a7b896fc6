"""The reference's encoder-analysis arithmetic restated in numpy (checker only): the downsample pyramid and the SAD scan.

  downsample         schro_frame_component_downsample, schroframe.c:1449-1505
  edgeextend         schro_frame_mc_edgeextend, schroframe.c:1940-1997
  scan_setup         schro_metric_scan_setup, schrometric.c:174-214
  do_scan, get_min   schro_metric_scan_do_scan / schro_metric_scan_get_min, schrometric.c:31-71, :121-171 (luma only)
  rough_scan_nohint  schro_rough_me_heirarchical_scan_nohint, schroroughmotion.c:64-141

tests/test_analysis_ref.py pins `downsample` and the SADs of `do_scan` on the reference's compiled kernels
(orc_downsample_vert_u8 / _horiz_u8, orc_sad_*: `downsample_orc`, `sad_orc` below drive them in the reference's own row
schedule where oracle/_ref is built) and on tests/golden/analysis_ref.npz everywhere.

What stays UNPINNED: schro_metric_scan_setup, schro_metric_scan_get_min and the loop of schroroughmotion.c cannot be
compiled here (the full library needs liborc), so `scan_setup`, `get_min` and `rough_scan_nohint` rest on this
restatement of their C text alone; so does `edgeextend` (a coordinate clamp)."""
import ctypes as C

import numpy as np

import oracle_lib as O

LIMIT_METRIC_SCAN = 42          # schrometric.h:16
METRIC_INVALID = 0x7fffffff     # SCHRO_METRIC_INVALID = INT_MAX, schrometric.h:55


def _filter(a, b, c, d):
    return (6 * (a + d) + 26 * (b + c) + 32) >> 6


def downsample(plane):
    """u8 h x w -> ceil (h / 2) x ceil (w / 2): the column pass rounded to u8 first, then the row pass."""
    p = np.asarray(plane, np.uint8).astype(np.int32)
    h, w = p.shape
    i = 2 * np.arange((h + 1) // 2)
    r = [np.clip(i + k, 0, h - 1) for k in (-1, 0, 1, 2)]
    tmp = _filter(p[r[0]], p[r[1]], p[r[2]], p[r[3]])
    assert tmp.max() <= 255
    tmp = tmp.astype(np.uint8).astype(np.int32)         # the u8 intermediate row (convwb)
    j = 2 * np.arange((w + 1) // 2)
    c = [np.clip(j + k, 0, w - 1) for k in (-1, 0, 1, 2)]
    d = _filter(tmp[:, c[0]], tmp[:, c[1]], tmp[:, c[2]], tmp[:, c[3]])
    assert d.max() <= 255
    return d.astype(np.uint8)


def edgeextend(plane, ext):
    """The picture with `ext` apron samples on every side, each the sample at the clamped coordinate."""
    return np.pad(np.asarray(plane), int(ext), mode="edge") if ext > 0 else np.asarray(plane).copy()


def pyramid(plane, levels):
    out = [np.asarray(plane, np.uint8)]
    for _ in range(levels):
        out.append(downsample(out[-1]))
    return out


def scan_setup(x, y, block_width, block_height, frame_width, frame_height, extension, dx, dy, dist):
    """(ref_x, ref_y, scan_width, scan_height), taken literally: the sizes may be <= 0."""
    assert dist > 0
    xmin = max(-block_width, x + dx - dist)
    xmax = min(frame_width, x + dx + dist)
    ymin = max(-block_height, y + dy - dist)
    ymax = min(frame_height, y + dy + dist)
    xmin = max(xmin, -extension)
    ymin = max(ymin, -extension)
    xmax = min(xmax, frame_width - block_width + extension)
    ymax = min(ymax, frame_height - block_height + extension)
    return xmin, ymin, xmax - xmin + 1, ymax - ymin + 1


def block_at(plane, x, y, bw, bh):
    """bh x bw samples from (x, y), coordinates clamped (the edge-extended apron)."""
    h, w = plane.shape
    ys = np.clip(np.arange(y, y + max(bh, 0)), 0, h - 1)
    xs = np.clip(np.arange(x, x + max(bw, 0)), 0, w - 1)
    return plane[np.ix_(ys, xs)]


def do_scan(frame, ref, s):
    """metrics[i * scan_height + j] (uint32) of scan `s` (a record or dict with the members of SchroHipMetricScan)."""
    bw, bh, sw, sh = int(s["block_width"]), int(s["block_height"]), int(s["scan_width"]), int(s["scan_height"])
    assert sw > 0 and sh > 0
    if bw <= 0 or bh <= 0:
        return np.zeros(sw * sh, np.uint32)
    blk = block_at(frame, int(s["x"]), int(s["y"]), bw, bh).astype(np.int32)
    win = block_at(ref, int(s["ref_x"]), int(s["ref_y"]), bw + sw - 1, bh + sh - 1).astype(np.int32)
    v = np.lib.stride_tricks.sliding_window_view(win, (bh, bw))         # [j, i, rows, cols]
    sad = np.abs(v - blk).sum(axis=(2, 3))
    return np.ascontiguousarray(sad.T).reshape(-1).astype(np.uint32)


def get_min(metrics, s):
    """(dx, dy, metric): starts at the gravity position, replaced by a strictly smaller metric, i outer, j inner."""
    sw, sh = int(s["scan_width"]), int(s["scan_height"])
    dx, dy = int(s["dx"]), int(s["dy"])
    i = int(s["gravity_x"]) + int(s["x"]) - int(s["ref_x"])
    j = int(s["gravity_y"]) + int(s["y"]) - int(s["ref_y"])
    assert 0 <= i < sw and 0 <= j < sh
    m = int(metrics[j + i * sh])
    for i in range(sw):
        for j in range(sh):
            v = int(metrics[i * sh + j])
            if v < m:
                m, dx, dy = v, int(s["ref_x"]) + i - int(s["x"]), int(s["ref_y"]) + j - int(s["y"])
    return dx, dy, m


def rough_scan_nohint(frame, ref, params, shift, distance, ref_index, extension=0):
    """The motion field of schro_rough_me_heirarchical_scan_nohint (O.MV_DTYPE records, x_num_blocks * y_num_blocks);
    frame and ref are the luma planes at pyramid level `shift`, `extension` their frames' apron."""
    nbx, nby, xb, yb = (int(params[k]) for k in ("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"))
    h, w = frame.shape
    mvs = np.zeros(nbx * nby, O.MV_DTYPE)
    mvs["flags"] = 1            # schro_motion_field_set (mf, 0, 1): pred_mode 1, split 0
    skip = 1 << shift
    for j in range(0, nby, skip):
        for i in range(0, nbx, skip):
            s = dict(x=(i >> shift) * xb, y=(j >> shift) * yb)
            s["block_width"], s["block_height"] = min(w - s["x"], xb), min(h - s["y"], yb)
            s["ref_x"], s["ref_y"], s["scan_width"], s["scan_height"] = scan_setup(
                s["x"], s["y"], s["block_width"], s["block_height"], w, h, extension, 0, 0, distance)
            s["dx"] = s["gravity_x"] = s["ref_x"] - s["x"]
            s["dy"] = s["gravity_y"] = s["ref_y"] - s["y"]
            mv = mvs[j * nbx + i]
            if s["scan_width"] <= 0 or s["scan_height"] <= 0:
                mv["v"][0] = mv["v"][2] = 0
                mv["metric"] = METRIC_INVALID
                continue
            dx, dy, m = get_min(do_scan(frame, ref, s), s)
            mv["metric"] = m
            mv["v"][ref_index] = np.int16(dx << shift)
            mv["v"][2 + ref_index] = np.int16(dy << shift)
    return mvs


# ---- the same through the reference's compiled kernels (oracle/_ref) --------------------------------------------------

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def downsample_orc(plane):
    """schro_frame_component_downsample with orc_downsample_vert_u8 / orc_downsample_horiz_u8 in its own row schedule:
    a vertical pass per destination row into a u8 row, then downsample_horiz_u8's three code paths."""
    L = O.reforc()
    src = np.ascontiguousarray(plane, np.uint8)
    h, w = src.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    dest = np.zeros((dh, dw), np.uint8)
    tmp = np.zeros(w + 8, np.uint8)

    def tap(i):
        t = tmp.astype(np.int32)
        x = sum(k * t[min(max(2 * i + o, 0), w - 1)] for k, o in ((6, -1), (26, 0), (26, 1), (6, 2)))
        return min(max((x + 32) >> 6, 0), 255)

    for r in range(dh):
        rows = [src[min(max(2 * r + k, 0), h - 1)] for k in (-1, 0, 1, 2)]
        L.orc_downsample_vert_u8(_p(tmp), _p(rows[0]), _p(rows[1]), _p(rows[2]), _p(rows[3]), C.c_int(w))
        if dw < 4:
            for i in range(dw):
                dest[r, i] = tap(i)
        else:
            dest[r, 0] = tap(0)
            n = w // 2 - 2
            if n > 0:
                L.orc_downsample_horiz_u8(C.c_void_p(dest[r].ctypes.data + 1), _p(tmp), C.c_int(n))
            for i in range(w // 2 - 2, dw):
                dest[r, i] = tap(i)
    return dest


def sad_orc(a, a_stride, b, b_stride, width, height):
    """schro_metric_absdiff_u8 (schrometric.c:10-29): the kernel the reference picks for the block size."""
    L = O.reforc()
    m = C.c_uint32(0)
    if height == 8 and width == 8:
        L.orc_sad_8x8_u8(C.byref(m), a, a_stride, b, b_stride)
    elif height == 12 and width == 12:
        L.orc_sad_12x12_u8(C.byref(m), a, a_stride, b, b_stride)
    elif width == 16:
        L.orc_sad_16xn_u8(C.byref(m), a, a_stride, b, b_stride, height)
    elif width == 32:
        L.orc_sad_32xn_u8(C.byref(m), a, a_stride, b, b_stride, height)
    else:
        L.orc_sad_nxm_u8(C.byref(m), a, a_stride, b, b_stride, width, height)
    return m.value


def do_scan_orc(frame, ref, s, extension):
    """schro_metric_scan_do_scan on an edge-extended copy of `ref` (and of `frame`), the SADs by the compiled kernels."""
    bw, bh, sw, sh = int(s["block_width"]), int(s["block_height"]), int(s["scan_width"]), int(s["scan_height"])
    e = int(extension) + 64
    f, r = np.ascontiguousarray(edgeextend(frame, e)), np.ascontiguousarray(edgeextend(ref, e))

    def at(a, x, y):
        return C.c_void_p(a.ctypes.data + (y + e) * a.strides[0] + (x + e))

    out = np.zeros(sw * sh, np.uint32)
    for i in range(sw):
        for j in range(sh):
            out[i * sh + j] = sad_orc(at(f, int(s["x"]), int(s["y"])), f.strides[0],
                                      at(r, int(s["ref_x"]) + i, int(s["ref_y"]) + j), r.strides[0], bw, bh)
    return out


# ---- the cases of tests/golden/analysis_ref.npz (tests/golden/make_analysis_golden.py, tests/test_analysis_ref.py) -----

GOLDEN_SIZES = [(1, 1), (2, 2), (3, 5), (7, 8), (8, 8), (9, 7), (17, 33), (64, 48)]     # (w, h)
GOLDEN_BLOCKS = [(8, 8), (12, 12), (16, 16), (16, 5), (32, 32), (5, 3), (4, 4)]          # (w, h)


def picture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def checkerboard(w, h):
    """0 / 255 squares of one sample: the largest steps the filter meets, at every edge phase."""
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * 255).astype(np.uint8)


def golden_scans():
    """[(frame, ref, scan, extension)]: every golden block size at a corner of a 72 x 56 picture (windows reaching into
    the apron) and inside it."""
    w, h, ext = 72, 56, 8
    frame, ref = picture(w, h, 501), picture(w, h, 502)
    out = []
    for n, (bw, bh) in enumerate(GOLDEN_BLOCKS):
        for (x, y, dist) in ((0, 0, 4), (w - bw, h - bh, 3), (20, 12, 2)):
            s = dict(x=x, y=y, block_width=bw, block_height=bh, dx=0, dy=0)
            s["ref_x"], s["ref_y"], s["scan_width"], s["scan_height"] = scan_setup(x, y, bw, bh, w, h, ext, 0, 0, dist)
            s["gravity_x"], s["gravity_y"] = s["ref_x"] - x, s["ref_y"] - y
            out.append((frame, ref, s, ext))
    return out
