"""Checker only (numpy): the reference's picture statistics restated -- the sums under the average luma and the squared
error, generate_coeff, the recursive Gaussian low-pass schro_frame_filter_lowpass2, the SSIM chain of schro_frame_ssim
with its per-pixel map and mssim, and the scene-change score.

What is pinned, and on what:
  * the per-row sums (orc_sum_u8, orc_sum_s16, orc_sum_square_diff_u8) on the reference's own compiled functions in
    oracle/_ref/libschroorc_ref.so, where that library is built (tests/test_picture_stats_ref.py), and on hand-derived
    values everywhere;
  * the vectorised low-pass (lowpass2) on the plain scalar transcription of the C loops (lowpass2_scalar), both in this
    file;
  * the SSIM high-pass (hipass: the u8 -> s16 conversion takes 128 off, then the low-pass is subtracted) on the compiled
    orc_offsetconvert_s16_u8 and orc_subtract_s16_u8, and it and the clamped products (multiply_s16) on hand-derived values.
What rests on the C text alone (schrofilter.c:516-814, schrossim.c:9-149, schroframe.c:1647-1680, schroanalysis.c:44-84,
schroengine.c:327-336): everything else.  schrofilter.c and schrossim.c cannot be compiled in this repository's oracle
build, so the low-pass and SSIM have no compiled twin.  Two readings in particular are the x86-64 build's and UNPINNED:
  * out of range -- `d[i] = rint (x)` into a uint8_t / int16_t converts the double to int32 (cvttsd2si; INT_MIN for
    what int32 does not hold) and keeps the low 8 / 16 bits (to_sample);
  * no contraction -- a step is four rounded products and three rounded sums in IEEE double, left to right (SSE2 has no
    fused multiply-add; a build with -march=haswell and -ffp-contract=fast could differ).
numpy evaluates `c0 * s + c1 * i0 + c2 * i1 + c3 * i2` as separate rounded operations, and so does CPython."""
import math

import numpy as np

INT32_MIN = -(1 << 31)


# ---- sums --------------------------------------------------------------------------------------------------------------

def _wrap32(v):
    return ((int(v) + (1 << 31)) & 0xffffffff) - (1 << 31)


def orc_sum_u8(row):
    """schroorc-dist.c:9361-9384: convubw, convuwl, accl into an int32."""
    return _wrap32(np.asarray(row, np.uint8).astype(np.int64).sum())


def orc_sum_s16(row):
    """:9439-9459: convswl, accl."""
    return _wrap32(np.asarray(row, np.int16).astype(np.int64).sum())


def orc_sum_square_diff_u8(a, b):
    """:9511-9548: subw on the zero-extended bytes, mullw (the low 16 bits of the product), convuwl, accl.  |a - b| <= 255
    and 255^2 = 65025 < 65536: the mask never removes a bit."""
    d = np.asarray(a, np.uint8).astype(np.int64) - np.asarray(b, np.uint8).astype(np.int64)
    sq = (d * d) & 0xffff
    assert np.array_equal(sq, d * d)
    return _wrap32(sq.sum())


def plane_sums(a, b=None):
    """The exact sums of the plane layer: (sum of a, sum of (a - b)^2 or 0) as Python ints."""
    a64 = np.asarray(a).astype(np.int64)
    s = int(a64.sum())
    if b is None:
        return s, 0
    d = a64 - np.asarray(b).astype(np.int64)
    return s, int((d * d).sum())


def average_luma(plane):
    """schro_frame_calculate_average_luma (schroframe.c:1647-1680): the rows' int32 sums into an `int`, which wraps;
    n = height * width."""
    plane = np.asarray(plane)
    row = orc_sum_u8 if plane.dtype == np.uint8 else orc_sum_s16
    total = 0
    for r in plane:
        total = _wrap32(total + row(r))
    return float(total) / _wrap32(plane.shape[0] * plane.shape[1])


def average_luma_of_sum(exact_sum, width, height):
    """The same from a plane's exact sum: the wraps of the rows and of the total are one wrap modulo 2^32."""
    return float(_wrap32(exact_sum)) / _wrap32(width * height)


def mean_squared_error(a_planes, b_planes):
    """schro_frame_mean_squared_error (schroanalysis.c:44-84): the rows' int32 sums added as doubles, over n as an int."""
    out = []
    for a, b in zip(a_planes, b_planes):
        s = 0.0
        for ra, rb in zip(a, b):
            s += float(orc_sum_square_diff_u8(ra, rb))
        out.append(s / float(_wrap32(a.shape[0] * a.shape[1])))
    return out


def scene_change_score(average, plane1, plane2):
    """schroengine.c:327-336."""
    luma = average - 16.0
    if luma > 0.01:
        return mean_squared_error([plane1], [plane2])[0] / (luma * luma)
    return 1.0


# ---- the low-pass ------------------------------------------------------------------------------------------------------

def generate_coeff(sigma):
    """schrofilter.c:666-689, statement by statement."""
    if sigma >= 2.5:
        q = 0.98711 * sigma - 0.96330
    else:
        q = 3.97156 - 4.41554 * math.sqrt(1 - 0.26891 * sigma)
    b0 = 1.57825 + 2.44413 * q + 1.4281 * q * q + 0.422205 * q * q * q
    b0inv = 1.0 / b0
    b1 = 2.44413 * q + 2.85619 * q * q + 1.26661 * q * q * q
    b2 = -1.4281 * q * q - 1.26661 * q * q * q
    b3 = 0.422205 * q * q * q
    B = 1 - (b1 + b2 + b3) / b0
    return [B, b1 * b0inv, b2 * b0inv, b3 * b0inv]


def to_sample(x, dtype):
    """`d = rint (x)` of the x86-64 build on an array of doubles: (stored samples, how many left the type's range)."""
    dtype = np.dtype(dtype)
    with np.errstate(invalid="ignore"):
        r = np.rint(x)
        inside = (r >= -2147483648.0) & (r < 2147483648.0)
    v = np.where(inside, r, float(INT32_MIN)).astype(np.int64)
    if dtype == np.uint8:
        d = v & 0xff
    else:
        d = ((v & 0xffff) ^ 0x8000) - 0x8000
    return d.astype(dtype), int(np.count_nonzero(d != v))


def _pass(lines, start, coeff, dtype, order):
    """One pass over `lines` (an (n, m) array: step k reads lines[k], m recursions side by side), in `order`."""
    c0, c1, c2, c3 = coeff
    i0 = start.astype(np.float64)
    i1, i2 = i0.copy(), i0.copy()
    bad = 0
    for k in order:
        x = c0 * lines[k].astype(np.float64) + c1 * i0 + c2 * i1 + c3 * i2
        i2, i1, i0 = i1, i0, x
        lines[k], n = to_sample(x, dtype)
        bad += n
    return bad


def lowpass2(plane, h_coeff, v_coeff):
    """schro_frame_component_filter_lowpass2_u8 / _s16 (schrofilter.c:691-782), vectorised over the rows, then over the
    columns: (filtered plane, out-of-range samples of the four passes)."""
    out = np.array(plane, copy=True)
    h, w = out.shape
    cols = out.T                        # a view: cols[x] is column x
    bad = _pass(cols, cols[0], h_coeff, out.dtype, range(w))            # every row forward: state s[0]
    bad += _pass(cols, cols[w - 1], h_coeff, out.dtype, range(w - 1, -1, -1))   # ... in reverse: state d[n - 1]
    bad += _pass(out, out[0], v_coeff, out.dtype, range(h))             # the columns forward: row 0 as the rows left it
    bad += _pass(out, out[h - 1], v_coeff, out.dtype, range(h - 1, -1, -1))     # ... in reverse: the last row
    return out, bad


def _rint_store(x, dtype):
    """to_sample for one Python float."""
    if math.isnan(x) or math.isinf(x):
        v = INT32_MIN
    else:
        v = round(x)                    # half to even, exact
        if not (-(1 << 31) <= v < (1 << 31)):
            v = INT32_MIN
    d = v & 0xff if dtype == np.uint8 else ((v & 0xffff) ^ 0x8000) - 0x8000
    return d, int(d != v)


def lowpass2_scalar(plane, h_coeff, v_coeff):
    """The same as a plain transcription of the C loops (lowpass2_u8 / _s16, schro_iir3_*_f64, schro_iir3_across_*_f64)."""
    dtype = np.asarray(plane).dtype
    d = [[int(v) for v in row] for row in np.asarray(plane)]
    h, w = len(d), len(d[0])
    bad = 0

    def iir3(line, order, state, coeff):
        nonlocal bad
        for i in order:
            x = coeff[0] * line[i] + coeff[1] * state[0] + coeff[2] * state[1] + coeff[3] * state[2]
            state[2] = state[1]
            state[1] = state[0]
            state[0] = x
            line[i], n = _rint_store(x, dtype)
            bad += n

    for row in d:
        iir3(row, range(w), [float(row[0])] * 3, h_coeff)
        iir3(row, range(w - 1, -1, -1), [float(row[w - 1])] * 3, h_coeff)
    for order, first in ((range(h), 0), (range(h - 1, -1, -1), h - 1)):
        i1 = [float(v) for v in d[first]]
        i2, i3 = list(i1), list(i1)
        for j in order:
            for i in range(w):
                x = v_coeff[0] * d[j][i] + v_coeff[1] * i1[i] + v_coeff[2] * i2[i] + v_coeff[3] * i3[i]
                i3[i] = i2[i]
                i2[i] = i1[i]
                i1[i] = x
                d[j][i], n = _rint_store(x, dtype)
                bad += n
    return np.array(d, dtype=np.int64).astype(dtype), bad


def frame_lowpass2(planes, sigma, h_shift, v_shift):
    """schro_frame_filter_lowpass2 (schrofilter.c:784-814): [filtered Y, U, V]."""
    ch, cv = sigma / (1 << h_shift), sigma / (1 << v_shift)
    out = [lowpass2(planes[0], generate_coeff(sigma), generate_coeff(sigma))[0]]
    for k in (1, 2):
        out.append(lowpass2(planes[k], generate_coeff(ch), generate_coeff(cv))[0])
    return out


# ---- SSIM --------------------------------------------------------------------------------------------------------------

SSIM_SIGMA = 1.5


def hipass(a, a_low):
    """a_hipass of schro_frame_ssim: (a - 128) - a_lowpass, -383 .. 127."""
    return (np.asarray(a, np.uint8).astype(np.int32) - 128) - np.asarray(a_low, np.uint8).astype(np.int32)


def multiply_s16(p, q):
    """schro_frame_multiply_s16 (schrossim.c:24-54): the int product clamped to [-32768, 32767]."""
    return np.clip(np.asarray(p, np.int64) * np.asarray(q, np.int64), -32768, 32767).astype(np.int16)


def ssim_map(a, b):
    """The per-pixel values of schro_frame_ssim (schrossim.c:64-123) over two u8 luma planes: (map, the out-of-range counts
    of the five low-passes: a_lowpass, b_lowpass, ab, a^2, b^2)."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    c = generate_coeff((a.shape[1] / 256.0) * SSIM_SIGMA)
    a_low, n0 = lowpass2(a, c, c)
    b_low, n1 = lowpass2(b, c, c)
    # schro_frame_dup16 (schrossim.c:9-22) is schro_frame_convert into an s16 frame: convert_s16_u8 (schrovirtframe.c:
    # 1742-1750) -> orc_offsetconvert_s16_u8 (schroorc-dist.c:4364-4393) stores u8 - 128; schro_frame_subtract_s16_u8
    # (schroframe.c:1159-1182) then takes the u8 low-pass off that
    ah, bh = hipass(a, a_low), hipass(b, b_low)

    ab, n2 = lowpass2(multiply_s16(ah, bh), c, c)
    aa, n3 = lowpass2(multiply_s16(ah, ah), c, c)
    bb, n4 = lowpass2(multiply_s16(bh, bh), c, c)
    c1 = (0.01 * 255) * (0.01 * 255)
    c2 = (0.03 * 255) * (0.03 * 255)
    mu_x, mu_y = a_low.astype(np.int64), b_low.astype(np.int64)
    sx2, sy2, sxy = aa.astype(np.int64), bb.astype(np.int64), ab.astype(np.int64)
    ssim = (2 * mu_x * mu_y + c1) * (2 * sxy + c2) / ((mu_x * mu_x + mu_y * mu_y + c1) * (sx2 + sy2 + c2))
    return ssim, [n0, n1, n2, n3, n4]


def raster_sum(values):
    """One accumulator over the values in raster order (schrossim.c:99-123); np.cumsum adds sequentially."""
    return float(np.cumsum(np.asarray(values, np.float64).ravel())[-1])


def mssim(values):
    """:124."""
    return raster_sum(values) / (values.shape[0] * values.shape[1])


def mssim_bound(values):
    """What two orders of adding the same n doubles may differ by, over n, plus the division's rounding:
    2 (n - 1) 2^-53 mean |s_i| + 2^-52 |mssim|."""
    n = values.size
    return 2.0 * (n - 1) * 2.0 ** -53 * float(np.mean(np.abs(values))) + 2.0 ** -52 * abs(mssim(values))
