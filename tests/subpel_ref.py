"""The restatement of schro_encoder_motion_predict_subpel_deep (schromotionest.c:246-354) for one (picture, reference)
pair, line for line and in raster order, over numpy planes.

The reads are RAW reads of the four planes of the upsampled reference with real `extension`-wide aprons, built as
schro_upsampled_frame_upsample builds them (schroframe.c:2000-2030; oracle/oracle_frame.c:79-118,180-197 restates the
edge extensions): every edge extension also overwrites the last column, or the bottom row, with its source plane's.
tests/test_subpel_ref.py compares the planes with oracle_lib.UpComp.get sample for sample.  Every read asserts that it
stays inside the aprons.

Switches that exist only for CPU assertions.  tests/subpel_cases.py: `stale_neighbours=True` predicts from the vectors
as they were at the start of the pass (doubled), and `fused` scores as the correctly rounded lambda * error + entropy (what
a fused multiply-add would give).  tests/long_diagonal_cases.py: `stale_neighbours` as a predicate (i, j, ni, nj) makes
neighbour (ni, nj) of block (i, j), where it says so, the record as it was before the pass -- NOT doubled: what a device
that missed the neighbour's stores would read -- and `order="diagonal"` walks the anti-diagonals i + j, each from the
bottom row up (the opposite of raster), in place: a block reads only blocks of earlier diagonals."""
from fractions import Fraction

import numpy as np

import oracle_lib as O

# sp_matches, schromotionest.c:259-262
MATCHES = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def _int16(v):
    return ((int(v) + 0x8000) & 0xffff) - 0x8000


def _extend(interior, hsrc, vsrc, e):
    """schro_frame_mc_edgeextend_horiz (interior's plane, hsrc) then _vert (.., vsrc): hsrc -- the INTERIOR of the plane
    the left and right aprons come from, vsrc -- the EXTENDED plane the rows above and below come from (None: this one)."""
    h, w = interior.shape
    a = np.zeros((h + 2 * e, w + 2 * e), np.uint8)
    a[e:e + h, e:e + w] = interior
    a[e:e + h, :e] = hsrc[:, :1]
    a[e:e + h, e + w - 1:] = hsrc[:, w - 1:w]          # "Remember to overwrite the last horizontal pel"
    v = a if vsrc is None else vsrc
    top, bottom = v[e].copy(), v[e + h - 1].copy()
    a[:e] = top
    a[e + h:] = bottom
    a[e + h - 1] = bottom                               # "Copy the src into the bottom line of frame"
    return a


def up_planes(pic, ext):
    """The four planes of the upsampled component, each (h + 2 * ext) x (w + 2 * ext) with pixel (0, 0) at [ext, ext]."""
    up = O.UpComp(pic, ext=max(ext, 4))                 # (the interiors do not depend on the apron width)
    i0, i1, i2, i3 = (up.plane(k) for k in range(4))
    p0 = _extend(i0, i0, None, ext)
    p2 = _extend(i2, i2, p0, ext)
    p1 = _extend(i1, i0, None, ext)
    p3 = _extend(i3, i2, p1, ext)
    return [p0, p1, p2, p3]


class UpFrame:
    """schro_upsampled_frame_get_block_fast_precN (upframe, 0, ..) over up_planes; `stats` counts what the reads touch."""

    def __init__(self, pic, ext, stats=None):
        self.h, self.w = pic.shape
        self.ext = ext
        self.planes = up_planes(pic, ext)
        self.stats = stats if stats is not None else {}

    def raw(self, x, y, bw, bh):
        """__schro_upsampled_frame_get_subdata_prec1 (schroframe.c:2186-2200) and the bw x bh samples read through it."""
        i = ((y & 1) << 1) | (x & 1)
        x >>= 1
        y >>= 1
        e = self.ext
        assert -e <= x and x + bw <= self.w + e and -e <= y and y + bh <= self.h + e, ("a read leaves the aprons", x, y, bw, bh, self.w, self.h, e)
        s = self.stats
        s["apron_columns"] = s.get("apron_columns", 0) + int(x < 0 or x + bw > self.w)
        s["rows_beyond"] = s.get("rows_beyond", 0) + int(y + bh > self.h)
        s["rows_above"] = s.get("rows_above", 0) + int(y < 0)
        return self.planes[i][y + e:y + e + bh, x + e:x + e + bw].astype(np.int32)

    def prec3(self, x, y, bw, bh):
        """schro_upsampled_frame_get_block_fast_prec3 (schroframe.c:2288-2413)."""
        hx, hy, rx, ry = x >> 2, y >> 2, x & 3, y & 3
        case = (ry << 2) | rx
        if case == 0:
            return self.raw(hx, hy, bw, bh)
        if case in (2, 8):
            a = self.raw(hx, hy, bw, bh)
            b = self.raw(hx, hy + 1, bw, bh) if rx == 0 else self.raw(hx + 1, hy, bw, bh)
            return (a + b + 1) >> 1                     # avgub
        w00, w01, w10, w11 = (4 - ry) * (4 - rx), (4 - ry) * rx, ry * (4 - rx), ry * rx
        v = (w00 * self.raw(hx, hy, bw, bh) + w01 * self.raw(hx + 1, hy, bw, bh) + w10 * self.raw(hx, hy + 1, bw, bh)
             + w11 * self.raw(hx + 1, hy + 1, bw, bh) + 8) >> 4
        return np.clip(v, 0, 255)                       # orc_combine4_nxm_u8 (schroorc.orc:1635-1662): convsuswb

    def block(self, x, y, prec, bw, bh):
        if prec == 1:
            return self.raw(x, y, bw, bh)
        if prec == 2:
            self.stats.setdefault("positions2", set()).add((x & 1, y & 1))
            return self.prec3(x << 1, y << 1, bw, bh)
        assert prec == 3
        self.stats.setdefault("positions3", set()).add((x & 3, y & 3))
        return self.prec3(x, y, bw, bh)


def estimate_sint(value):
    """schro_pack_estimate_sint (schropack.c:204-226)."""
    value = abs(int(value))
    n_bits = (value + 1).bit_length()                   # maxbit (value + 1)
    n_bits = n_bits + n_bits - 1
    return n_bits + 1 if value else n_bits


def _median3(a, b, c):
    return sorted((a, b, c))[1]


def vector_prediction(v, nbx, x, y, ref):
    """schro_mf_vector_prediction (schromotion.c:259-312) over the (records, 4) vector array v."""
    vx, vy = [], []
    for cond, k in ((x > 0, y * nbx + x - 1), (y > 0, (y - 1) * nbx + x), (x > 0 and y > 0, (y - 1) * nbx + x - 1)):
        if cond:
            vx.append(int(v[k][ref]))
            vy.append(int(v[k][2 + ref]))
    n = len(vx)
    if n == 0:
        return 0, 0
    if n == 1:
        return vx[0], vy[0]
    if n == 2:
        return (vx[0] + vx[1] + 1) >> 1, (vy[0] + vy[1] + 1) >> 1
    return _median3(*vx), _median3(*vy)


def _score(entropy, lam, error, fused):
    if fused:
        return float(Fraction(lam) * int(error) + entropy)
    return entropy + lam * float(error)                 # a rounded product, then a rounded sum


def block_order(nbx, nby, order):
    """The blocks (i, j) line by line: the rows of the C loops, or the anti-diagonals."""
    if order == "raster":
        return [[(i, j) for i in range(nbx)] for j in range(nby)]
    assert order == "diagonal"
    return [[(d - j, j) for j in range(min(d, nby - 1), max(0, d - (nbx - 1)) - 1, -1)] for d in range(nbx + nby - 1)]


def subpel_deep(src, ref, params, mv_precision, ref_index, lam, field, extension, tables=None, stale_neighbours=False,
                fused=False, stats=None, order="raster"):
    """(field, [the int32 (records, 8) error table of pass 1, 2, ..]).  src, ref: the luma planes (ref may be None with
    `tables`); field: the MV_DTYPE source field (not changed); tables: the error tables to choose from instead of the
    pictures (-1: inadmissible), one per pass."""
    nbx, nby, xblen, yblen = (params[k] for k in ("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"))
    height, width = src.shape
    st = stats if stats is not None else {}
    for key in ("skipped", "clipped", "inadmissible", "ties", "shifted"):
        st.setdefault(key, 0)
    st.setdefault("wins", [0] * 9)
    upframe = UpFrame(ref, extension, st) if tables is None else None
    mf = field.copy()                                   # "the destination is first a copy of the source"
    v = mf["v"]
    out = []
    x_min = y_min = -extension
    mvprec = 0
    while True:
        mvprec += 1
        if mv_precision < mvprec:
            break
        x_max, y_max = (width << mvprec) + extension, (height << mvprec) + extension
        table = np.full((nbx * nby, 8), -1, np.int32)
        start = v.copy()
        for line in block_order(nbx, nby, order):
            for i, j in line:
                n = j * nbx + i
                # schro_frame_get_data (orig_frame, &orig, 0, i * xblen, j * yblen)
                if i * xblen >= width or j * yblen >= height:
                    st["skipped"] += 1
                    continue
                bw, bh = min(xblen, width - i * xblen), min(yblen, height - j * yblen)
                st["clipped"] += int(bw < xblen or bh < yblen)
                v[n][ref_index] = _int16(int(v[n][ref_index]) << 1)
                v[n][2 + ref_index] = _int16(int(v[n][2 + ref_index]) << 1)
                st["shifted"] += 1
                mvx, mvy = int(v[n][ref_index]), int(v[n][2 + ref_index])
                if callable(stale_neighbours):
                    vx, vy = [], []
                    for cond, ni, nj in ((i > 0, i - 1, j), (j > 0, i, j - 1), (i > 0 and j > 0, i - 1, j - 1)):
                        if cond:
                            rec = (start if stale_neighbours(i, j, ni, nj) else v)[nj * nbx + ni]
                            vx.append(int(rec[ref_index]))
                            vy.append(int(rec[2 + ref_index]))
                    pred_x, pred_y = ((0, 0) if not vx else (vx[0], vy[0]) if len(vx) == 1 else
                                      ((vx[0] + vx[1] + 1) >> 1, (vy[0] + vy[1] + 1) >> 1) if len(vx) == 2 else (_median3(*vx), _median3(*vy)))
                elif stale_neighbours:
                    stale = np.array([[_int16(int(a) << 1) for a in rec] for rec in start[[max(n - 1, 0), max(n - nbx, 0), max(n - nbx - 1, 0)]]])
                    vx, vy = [], []
                    for cond, k in ((i > 0, 0), (j > 0, 1), (i > 0 and j > 0, 2)):
                        if cond:
                            vx.append(int(stale[k][ref_index]))
                            vy.append(int(stale[k][2 + ref_index]))
                    pred_x, pred_y = ((0, 0) if not vx else (vx[0], vy[0]) if len(vx) == 1 else
                                      ((vx[0] + vx[1] + 1) >> 1, (vy[0] + vy[1] + 1) >> 1) if len(vx) == 2 else (_median3(*vx), _median3(*vy)))
                else:
                    pred_x, pred_y = vector_prediction(v, nbx, i, j, ref_index)
                entropy = estimate_sint(mvx - pred_x) + estimate_sint(mvy - pred_y)
                min_score = _score(entropy, lam, int(mf["metric"][n]), fused)
                min_error, m = None, -1
                x, y = i * (xblen << mvprec) + mvx, j * (yblen << mvprec) + mvy
                orig = src[j * yblen:j * yblen + bh, i * xblen:i * xblen + bw].astype(np.int32) if tables is None else None
                for k, (mdx, mdy) in enumerate(MATCHES):
                    dx, dy = x + mdx, y + mdy
                    if tables is None:
                        if not (x_min < dx) or not (x_max > dx + xblen - 1) or not (y_min < dy) or not (y_max > dy + yblen - 1):
                            st["inadmissible"] += 1
                            continue
                        error = int(np.abs(orig - upframe.block(dx, dy, mvprec, bw, bh)).sum())
                    else:
                        error = int(tables[mvprec - 1][n][k])
                        if error < 0:
                            st["inadmissible"] += 1
                            continue
                    table[n][k] = error
                    entropy = estimate_sint(mvx + mdx - pred_x) + estimate_sint(mvy + mdy - pred_y)
                    score = _score(entropy, lam, error, fused)
                    st["ties"] += int(score == min_score)
                    if min_score > score:
                        min_score, min_error, m = score, error, k
                st["wins"][m + 1] += 1                  # entry 0: none
                if m != -1:
                    v[n][ref_index] = _int16(mvx + MATCHES[m][0])
                    v[n][2 + ref_index] = _int16(mvy + MATCHES[m][1])
                    mf["metric"][n] = min_error
        out.append(table)
    return mf, out
