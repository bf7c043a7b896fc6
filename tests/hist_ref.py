"""The checker of the sub-band histograms (schro_hip_histogram_batch, schro_hipframe_subband_histograms): a numpy
restatement of the reference's C text -- schrohistogram.c:11-22 (ilogx), :148-173 (add, add_array_s16, scale), :345-391
(the plain and the DC-predict form) and schroquantiser.c:600-637 (which form and which skip a sub-band takes).  That file
is not among the sources the oracle recipe compiles, so nothing here is pinned on a compiled reference: it is held by
tests/test_hist_ref.py (properties of ilogx over every s16 value, the four prediction cases by hand, schro_divide3's
range, a scalar loop transcribed line by line) -- the role tests/quant_ref.py plays for the quantiser's DC recurrence.

One departure, the device's: the reference indexes bins[ilogx (v)] without a bound; here, as there, every sample whose
index is >= 104 is counted in `overflow` and the bins stay as they are.  s32 samples (the reference reads s16 only) take
the same expressions in 32-bit wrapping ints."""
import numpy as np

BINS = 104                      # SCHRO_HISTOGRAM_SIZE: (16 - SHIFT) * (1 << SHIFT), SHIFT = 3


def wrap32(a):
    """an int64 array as C's int would hold it after 32-bit wrapping arithmetic"""
    return ((np.asarray(a, np.int64) + (1 << 31)) & 0xffffffff) - (1 << 31)


def ilogx(v):
    """x = |v|; while x >= 16: x >>= 1, i++; x + 8 i.  Vectorised; int64 in, int64 out (unbounded: 104 and up for
    |v| >= 32768)."""
    x = np.abs(np.asarray(v, np.int64))
    i = np.zeros_like(x)
    while True:
        m = x >= 16
        if not m.any():
            return x + 8 * i
        x = np.where(m, x >> 1, x)
        i += m


def ilogx_size(i):
    """how many values of |v| share bin i"""
    return 1 if i < 8 else 1 << ((i >> 3) - 1)


def divide3(a):
    """schro_divide3: (a * 21845 + 10922) >> 16 in 32-bit int"""
    return wrap32(wrap32(a) * 21845 + 10922) >> 16


def dc_differences(band):
    """line[i] - pred of every sample of a band (h x w), pred from the ORIGINAL neighbours: 0 at (0, 0), the left
    neighbour on row 0, the upper one in column 0, else schro_divide3 (left + up + upleft + 1)."""
    b = np.asarray(band).astype(np.int64)
    pred = np.zeros_like(b)
    pred[0, 1:] = b[0, :-1]
    pred[1:, 0] = b[:-1, 0]
    pred[1:, 1:] = divide3(wrap32(b[1:, :-1] + b[:-1, 1:] + b[:-1, :-1] + 1))
    return wrap32(b - pred)


def counts(band, skip=1, dc=False):
    """The raw counts of a band's sampled rows (0, skip, 2 skip ...): a uint32 array of 105 -- 104 bins, then overflow."""
    band = np.asarray(band)
    if band.size == 0:
        return np.zeros(BINS + 1, np.uint32)
    v = dc_differences(band) if dc else band.astype(np.int64)
    idx = np.minimum(ilogx(v[::skip]), BINS)
    return np.bincount(idx.reshape(-1), minlength=BINS + 1).astype(np.uint32)


def histogram(band, skip=1, dc=False):
    """(n, bins, overflow) as schro_frame_data_generate_histogram[_dc_predict] + schro_histogram_scale leave them:
    n = sampled values x skip (int), bins float64 = counts x skip; overflow = the overflow count x skip."""
    c = counts(band, skip, dc)
    band = np.asarray(band)
    sampled = band[::skip].size if band.size else 0
    return int(sampled * skip), c[:BINS].astype(np.float64) * skip, int(c[BINS]) * skip


def position(index):
    """schro_subband_get_position"""
    return 0 if index == 0 else (((index - 1) // 3) << 2) | ((index - 1) % 3 + 1)


def band_skip(index):
    """skip = 1 << MAX (0, SCHRO_SUBBAND_SHIFT (position) - 1)"""
    return 1 << max(0, (position(index) >> 2) - 1)


def band_rect(width, height, depth, index, stride, itemsize):
    """schro_subband_get_frame_data (schroparams.c:319-352): (byte offset, stride in bytes, width, height) of sub-band
    `index` of a width x height transform of `depth` levels whose rows are `stride` bytes apart."""
    pos = position(index)
    shift = depth - (pos >> 2)
    bw, bh, bstride = width >> shift, height >> shift, stride << shift
    return ((bstride >> 1) if pos & 2 else 0) + (bw * itemsize if pos & 1 else 0), bstride, bw, bh


def band_view(plane, depth, index):
    """sub-band `index` of a coefficient plane (h x w array, in-place layout) as an array"""
    h, w = plane.shape
    off, stride, bw, bh = band_rect(w, h, depth, index, w, 1)
    y0, x0 = divmod(off, w)
    step = stride // w
    return plane[y0::step, x0:x0 + bw][:bh]


def frame_histograms(planes, depth, intra):
    """schro_encoder_generate_subband_histograms over the three coefficient planes: lists of n, bins (float64 rows) and
    overflow, component-major, sub-band index minor."""
    ns, bins, ovf = [], [], []
    for p in planes:
        for i in range(1 + 3 * depth):
            n, b, o = histogram(band_view(p, depth, i), band_skip(i), dc=bool(intra) and i == 0)
            ns.append(n)
            bins.append(b)
            ovf.append(o)
    return np.array(ns, np.int64), np.array(bins, np.float64), np.array(ovf, np.uint32)
