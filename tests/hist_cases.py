"""Shared by tests/test_gpu_histogram.py, tests/test_histogram_api.py and tests/dry_run_hist_cases.py: bands as records, the
runner that compares a schro_hip_histogram_batch call with tests/hist_ref.py count for count, frame-layer pictures and the
refusal cases."""
import ctypes as C

import numpy as np

import hist_ref as H
from schroedinger_amd import _lib, frames

EINVAL = -1


def band_array(buf, band):
    """the samples of band (offset, stride, width, height, ...) -- bytes, bytes, samples, samples -- of the plane `buf`
    (a C-contiguous 2-D array: its rows ARE the plane's pitch)"""
    off, stride, w, h = band[:4]
    b = buf.dtype.itemsize
    flat = buf.reshape(-1)
    assert off % b == 0 and stride % b == 0 and off // b + (h - 1) * (stride // b) + w <= flat.size
    return np.lib.stride_tricks.as_strided(flat[off // b:], shape=(h, w), strides=(stride, b), writeable=False)


def expected(spec):
    """(nbands, 105) uint32: the raw counts of a spec's bands by tests/hist_ref.py"""
    return np.stack([H.counts(band_array(spec["buf"], bd), bd[4], bool(bd[5])) for bd in spec["bands"]])


def sub_band(buf, y0, x0, w, h, skip=1, dc=0, row_step=1):
    """a band record for the w x h rectangle at (y0, x0) of `buf`, its rows row_step plane rows apart"""
    b, pitch = buf.dtype.itemsize, buf.shape[1]
    return ((y0 * pitch + x0) * b, pitch * b * row_step, w, h, skip, dc)


def run_specs(ctx, specs):
    """One schro_hip_histogram_batch call over all specs (dict(buf=plane array, bands=[records])), compared with the
    checker.  The planes are uploaded tight (stride = the array's row), so a band may start at any sample.  Returns the
    counts."""
    planes = [ctx.upload(s["buf"], stride=s["buf"].shape[1] * s["buf"].dtype.itemsize) for s in specs]
    got = ctx.histogram_batch([(p, s["bands"]) for p, s in zip(planes, specs)])
    for n, (s, g) in enumerate(zip(specs, got)):
        want = expected(s)
        assert g.shape == want.shape and g.dtype == np.uint32
        bad = np.argwhere(g != want)
        assert not len(bad), ("plane %d" % n, "first (band, bin):", bad[:4].tolist(), [(int(g[b, k]), int(want[b, k])) for b, k in bad[:4]])
    for p in planes:
        p.free()
    return got


def mixed_specs(dtype, seed):
    """three components x depth 3 of a 96 x 64 and a 50 x 38 picture (4:2:0; the second one's sizes are what they are:
    bands of 6 x 4, 3 x 2 ... and odd widths), sub-band 0 in the DC form for the first picture"""
    rng = np.random.default_rng(seed)
    b = np.dtype(dtype).itemsize
    specs = []
    for n, (w, h, intra) in enumerate(((96, 64, 1), (50, 38, 0))):
        for k in range(3):
            cw, ch = (w, h) if k == 0 else (w // 2, h // 2)
            pitch = cw + (3, 0, 1)[k]
            buf = coefficients(rng, (ch, pitch), dtype)
            bands = []
            for i in range(10):
                off, stride, bw, bh = H.band_rect(cw, ch, 3, i, pitch * b, b)
                if bw > 0 and bh > 0:
                    bands.append((off, stride, bw, bh, H.band_skip(i), int(intra and i == 0)))
            specs.append(dict(buf=buf, bands=bands))
    return specs


def coefficients(rng, shape, dtype, wide_every=5):
    """mostly small values (the low bins, where lanes meet), some over the whole 16-bit range and, on s32, beyond it"""
    small = np.rint(rng.laplace(0.0, 6.0, shape)).astype(np.int64)
    lim = 32768 if np.dtype(dtype) == np.int16 else 1 << 20
    wide = rng.integers(-lim, lim, shape)
    return np.where(rng.integers(0, wide_every, shape) == 0, wide, small).astype(dtype)


class FramePicture:
    """One picture for schro_hipframe_subband_histograms: its device frame and what tests/hist_ref.py expects."""

    def __init__(self, ctx, dtype, intra, w, h, depth, chroma_shift, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.depth, self.intra = ctx, depth, intra
        cw, ch = w >> chroma_shift, h >> chroma_shift
        self.planes = [coefficients(rng, s, dtype) for s in ((h, w), (ch, cw), (ch, cw))]
        fmt = frames.frame_format(dtype, chroma_shift, chroma_shift)
        self.iwt = frames.DeviceFrame(ctx, fmt, w, h).upload(frames.HostFrame(self.planes, chroma_shift, chroma_shift))
        self.params = frames.make_params(transform_depth=depth, num_refs=0 if intra else 1, iwt_luma_width=w, iwt_luma_height=h,
                                         iwt_chroma_width=cw, iwt_chroma_height=ch)

    def check(self, unref=True):
        n, bins, ovf = self.ctx.subband_histograms(self.iwt, self.params)
        wn, wbins, wovf = H.frame_histograms(self.planes, self.depth, self.intra)
        assert bins.dtype == np.float64 and bins.shape == wbins.shape
        assert np.array_equal(n, wn), ("n", n.tolist(), wn.tolist())
        assert np.array_equal(bins, wbins), ("bins", np.argwhere(bins != wbins)[:4].tolist())
        assert np.array_equal(ovf, wovf), ("overflow", ovf.tolist(), wovf.tolist())
        assert np.array_equal(n, bins.sum(axis=1) + ovf)
        if unref:
            self.iwt.unref()
        return n, bins, ovf


REFUSAL_PLANE = (16, 32)        # rows x samples of the s16 plane the refusal cases describe


def refusal_table(stride):
    """(good bands, cases) for a plane of REFUSAL_PLANE samples and `stride` bytes a row: name -> (the bad plane's bands and
    members, the words its message holds).  Read by refusal_cases below and by tests/encoder_walk_cases.py."""
    good = [(0, stride, 16, 16, 1, 0), (32, stride, 16, 16, 2, 1)]

    def rec(**kw):
        r = dict(off=0, stride=stride, w=16, h=16, skip=1, dc=0)
        r.update(kw)
        return [good[0], (r["off"], r["stride"], r["w"], r["h"], r["skip"], r["dc"])]

    cases = {
        "bad sample size": (dict(bands=good, bps=3), ("bytes_per_sample",)),
        "zero width": (dict(bands=rec(w=0)), ("plane 1", "band 1")),
        "negative height": (dict(bands=rec(h=-4)), ("plane 1", "band 1")),
        "skip zero": (dict(bands=rec(skip=0)), ("plane 1", "band 1", "skip")),
        "skip not a power of two": (dict(bands=rec(skip=3)), ("plane 1", "band 1", "skip")),
        "negative skip": (dict(bands=rec(skip=-2)), ("plane 1", "band 1", "skip")),
        "stride shorter than a row": (dict(bands=rec(stride=30)), ("plane 1", "band 1", "stride")),
        "stride not a multiple of the sample": (dict(bands=rec(stride=stride + 1)), ("plane 1", "band 1", "stride")),
        "band past the plane": (dict(bands=rec(off=stride * 8)), ("plane 1", "band 1", "outside")),
        "band past the plane's last row by one sample": (dict(bands=rec(off=34)), ("plane 1", "band 1", "outside")),
        "band starting in front of the plane": (dict(bands=rec(off=-2)), ("plane 1", "band 1", "outside")),
        "DC band whose row above would lie in front of the plane": (dict(bands=rec(off=-stride, dc=1)), ("plane 1", "band 1", "outside")),
        "offset not a multiple of the sample": (dict(bands=rec(off=1)), ("plane 1", "band 1", "outside")),
        "2^32 sampled values": (dict(bands=rec(w=1 << 16, h=1 << 16, stride=1 << 17), bytes=1 << 40), ("plane 1", "band 1", "sampled values")),
        "no bands": (dict(bands=good, nbands=0), ("plane 1",)),
        "no counts": (dict(bands=good, counts=None), ("plane 1",)),
    }
    return good, cases


def refusal_cases(ctx):
    """Every refusal of schro_hip_histogram_batch: SCHRO_HIP_EINVAL, nothing launched, the message naming plane and band.
    The planes are real allocations of the context (a call that wrongly went through would only touch them)."""
    lib = ctx.lib
    # what a call that enqueued its clear or its launch before it had validated everything would touch: the counts (of the
    # good planes in front of the bad one too) hold a sentinel, the coefficients known values, compared after every refusal
    coeffs = (np.arange(REFUSAL_PLANE[0] * REFUSAL_PLANE[1], dtype=np.int64).reshape(*REFUSAL_PLANE) * 37 % 2001 - 1000).astype(np.int16)
    co = ctx.upload(coeffs)
    cnt = ctx.plane(2, _lib.HISTOGRAM_BINS + 1, np.uint32, stride=C.sizeof(_lib.HistogramCounts)).fill(0xa5)
    sentinel = np.full((2, _lib.HISTOGRAM_BINS + 1), 0xa5a5a5a5, np.uint32)

    def unchanged(name):
        ctx.synchronize()
        assert np.array_equal(cnt.download(), sentinel), (name, "the counts were written")
        assert np.array_equal(co.download(), coeffs), (name, "the coefficients were written")
    good, cases = refusal_table(co.stride)

    def call(bands, bps=2, plane=1, **kw):
        """the bad plane is plane `plane` of the call, behind good ones"""
        arr = (_lib.HistogramPlane * (plane + 1))()
        keep = []
        for k in range(plane + 1):
            recs = bands if k == plane else good
            tab = (_lib.HistogramBand * len(recs))(*[_lib.HistogramBand(*r) for r in recs])
            keep.append(tab)
            a = arr[k]
            a.coeffs, a.bytes, a.bands, a.nbands, a.counts = co.ptr, co.stride * co.height, tab, len(tab), cnt.ptr
            if k == plane:
                for name, v in kw.items():
                    setattr(a, name, v)
        rc = lib.schro_hip_histogram_batch(ctx.h, arr, plane + 1, bps)
        msg = lib.schro_hip_last_error()
        return rc, (msg.decode() if msg else "")

    for name, (kw, words) in cases.items():
        rc, msg = call(**kw)
        assert rc == EINVAL, (name, rc, msg)
        assert "histogram_batch" in msg and all(w in msg for w in words), (name, msg)
        unchanged(name)
    assert lib.schro_hip_histogram_batch(None, None, 1, 2) == EINVAL and b"histogram_batch" in lib.schro_hip_last_error()
    unchanged("no context")
    # ... and the same planes, unspoilt, are taken: now the counts ARE written (the sentinel is gone), the coefficients not
    rc, msg = call(good)
    assert rc == 0, msg
    ctx.synchronize()
    assert not np.array_equal(cnt.download(), sentinel) and np.array_equal(co.download(), coeffs)
    for p in (co, cnt):
        p.free()
    return len(cases)
