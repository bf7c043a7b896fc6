"""GPU parity: the sub-band histograms (schro_hip_histogram_batch, schro_hipframe_subband_histograms) against
tests/hist_ref.py, count for count -- integers, so exactly.  The checker restates schrohistogram.c and is held by
tests/test_hist_ref.py."""
import ctypes as C

import numpy as np
import pytest

import guard_lib as G
import hist_cases as HC
import hist_ref as H
import schroedinger_amd as sa
from schroedinger_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [1] * 16 + [1 << ((i >> 3) - 1) for i in range(16, 104)]        # values of |v| per bin


def all_s16():
    return np.arange(-32768, 32768, dtype=np.int64).astype(np.int16).reshape(256, 256)


@pytest.mark.parametrize("skip", [1, 2])
def test_every_value(ctx, skip):
    """A 256 x 256 s16 band holding every value once: every bin gets its known size (twice: v and -v; once for 0), and
    -32768 is the one overflow.  skip 2: the even rows, i.e. the values -32768 + 512 r + c."""
    x = all_s16()
    (got,), = HC.run_specs(ctx, [dict(buf=x, bands=[HC.sub_band(x, 0, 0, 256, 256, skip=skip)])])
    if skip == 1:
        assert got[:104].tolist() == [1] + [2 * s for s in SIZES[1:]] and got[104] == 1
    assert int(got.sum()) == 65536 // skip and got[104] == 1


def test_contention(ctx):
    """All lanes of every wave on one bin: zeros (a bin counted in registers), one repeated non-zero value of a register
    bin and of an LDS bin, and two alternating values in a band 128 columns wide."""
    z = np.zeros((64, 64), np.int16)
    three, big = np.full((64, 64), -3, np.int16), np.full((64, 64), 1000, np.int16)
    alt = np.tile(np.array([0, 77], np.int16), (48, 64))
    alt2 = np.tile(np.array([[5, -9000], [-9000, 5]], np.int16), (24, 64))
    got = HC.run_specs(ctx, [dict(buf=b, bands=[HC.sub_band(b, 0, 0, b.shape[1], b.shape[0])]) for b in (z, three, big, alt, alt2)])
    assert got[0][0, 0] == 4096 and got[0][0].sum() == 4096
    assert got[1][0, 3] == 4096 and got[2][0, int(H.ilogx(1000))] == 4096
    assert got[3][0, 0] == got[3][0, int(H.ilogx(77))] == 48 * 64


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_geometry(ctx, dtype):
    """Widths 1 .. 130 (below, at and above a group, a wave's columns and the 64 / 65 boundary), heights 1 .. 9 with skips
    1, 2, 4 (height < skip, height no multiple of skip), strides wider than the row, bands starting at odd samples
    (2-byte-aligned starts on s16), more than one workgroup per band (130 x 130: 2210 groups on s16)."""
    rng = np.random.default_rng(7)
    pitch, rows = 141, 140
    buf = HC.coefficients(rng, (rows, pitch), dtype)
    bands = []
    for n, w in enumerate((1, 3, 5, 63, 64, 65, 130)):
        for m, h in enumerate((1, 2, 3, 7, 9)):
            for skip in (1, 2, 4):
                bands.append(HC.sub_band(buf, (3 * n + m) % 17, (n + m + skip) % 11, w, h, skip=skip))
    bands.append(HC.sub_band(buf, 1, 3, 130, 130, skip=1))
    bands.append(HC.sub_band(buf, 0, 1, 129, 69, skip=2, row_step=2))          # rows two plane rows apart
    # rows of more groups than a workgroup has lanes (263 on s16): a lane's next group lies in the same row
    wide = HC.coefficients(rng, (5, 2101), dtype)
    HC.run_specs(ctx, [dict(buf=buf, bands=bands[:40]), dict(buf=buf, bands=bands[40:]),
                       dict(buf=wide, bands=[HC.sub_band(wide, 0, 1, 2100, 5, skip=2), HC.sub_band(wide, 1, 0, 2099, 3, skip=1, dc=1)])])


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_dc_form(ctx, dtype):
    rng = np.random.default_rng(9)
    lim = 1 << (8 * np.dtype(dtype).itemsize - 1)
    specs = []
    for (w, h) in ((1, 1), (1, 5), (5, 1), (17, 9), (65, 33)):
        pitch = w + 3
        buf = HC.coefficients(rng, (h + 2, pitch), dtype)
        full = rng.integers(-lim, lim, (h + 2, pitch)).astype(dtype)            # differences over the whole range
        for b in (buf, full):
            # the band one row and one sample inside the plane: what lies above and to the left of it is never read
            specs.append(dict(buf=b, bands=[HC.sub_band(b, 1, 1, w, h, skip=s, dc=1) for s in (1, 2, 4)]))
    HC.run_specs(ctx, specs)


def test_dc_form_extremes_overflow_and_leave_the_bins_alone(ctx):
    """+-32767 and -32768 in a checkerboard: every difference but the first lies beyond 15 bits (the reference would write
    past its array, up to index 111): counted in overflow, no bin moves but the first sample's."""
    yy, xx = np.mgrid[0:33, 0:65]
    for lo in (-32767, -32768):
        b = np.where((yy + xx) & 1, lo, 32767).astype(np.int16)
        (got,), = HC.run_specs(ctx, [dict(buf=b, bands=[HC.sub_band(b, 0, 0, 65, 33, dc=1)])])
        # (0, 0) counts 32767 itself, bin 103; row 0 and column 0 differ by 65534 / 65535; inside, the prediction is the
        # third of two of one kind and one of the other: +-10922 or so against +-32767
        assert got[104] == 65 * 33 - 1 and got[103] == 1 and got[:103].sum() == 0


def test_mixed_batches_and_a_repeated_call(ctx):
    """One call over planes of unlike sizes, skips and forms; the same call again, nothing cleared by the caller."""
    for dtype in (np.int16, np.int32):
        specs = HC.mixed_specs(dtype, seed=13)
        assert len(specs) == 6 and any(bd[5] for s in specs for bd in s["bands"]) and {bd[4] for s in specs for bd in s["bands"]} == {1, 2}
        HC.run_specs(ctx, specs)
    planes = [ctx.upload(s["buf"], stride=s["buf"].shape[1] * s["buf"].dtype.itemsize) for s in specs]
    arr, counts, block = ctx.histogram_planes([(p, s["bands"]) for p, s in zip(planes, specs)])
    results = []
    for _ in range(3):
        sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, arr, len(specs), 4))
        results.append([c.download() for c in counts])
    for r in results:
        for got, s in zip(r, specs):
            assert np.array_equal(got, HC.expected(s))
    for p in planes + [block]:
        p.free()


def test_s32_values_beyond_16_bits(ctx):
    rng = np.random.default_rng(21)
    s16 = HC.coefficients(rng, (40, 70), np.int16)
    wide = s16.astype(np.int32)
    band = lambda b, dc: [HC.sub_band(b, 0, 0, 70, 40, skip=1, dc=dc), HC.sub_band(b, 0, 0, 70, 40, skip=2, dc=dc)]
    a, b_ = HC.run_specs(ctx, [dict(buf=s16, bands=band(s16, 0) + band(s16, 1))]), HC.run_specs(ctx, [dict(buf=wide, bands=band(wide, 0) + band(wide, 1))])
    assert np.array_equal(a[0], b_[0])                                  # within 16 bits: the s16 result, both forms
    big = np.array([[32768, -32768, 1 << 20, -(1 << 31), (1 << 31) - 1, 32767, -32767, 0, 15, 16]], np.int32)
    (got,), = HC.run_specs(ctx, [dict(buf=big, bands=[HC.sub_band(big, 0, 0, 10, 1)])])
    assert got[104] == 5 and got[103] == 2 and got[0] == 1 and got[15] == 1 and got[16] == 1


@pytest.mark.parametrize("dtype,shift", [(np.int16, 1), (np.int32, 1), (np.int16, 0)])
@pytest.mark.parametrize("intra", [0, 1])
def test_frame_layer(ctx, dtype, shift, intra):
    """depths 1, 3 and 4, 4:2:0 and 4:4:4: the geometry changes between the calls (the table is rebuilt), and comes back"""
    for (w, h, depth) in ((64, 48, 1), (96, 64, 3), (80, 48, 4), (96, 64, 3)):
        HC.FramePicture(ctx, dtype, intra, w, h, depth, shift, seed=3 + depth).check()


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("intra", [0, 1])
def test_frame_layer_sub_bands_of_no_size(ctx, dtype, intra):
    """8 x 8 4:2:0 at depth 3: the chroma LL, HL, LH and HH of the coarsest level are 0 x 0 -- all-zero histograms with
    n = 0, beside the luma's 1 x 1 bands and the other levels, which count as ever."""
    n, bins, ovf = HC.FramePicture(ctx, dtype, intra, 8, 8, 3, 1, seed=17).check()
    for comp in (1, 2):
        for i in range(4):
            k = comp * 10 + i
            assert n[k] == 0 and not bins[k].any() and ovf[k] == 0
    assert n[:4].tolist() == [1, 1, 1, 1] and n[10 + 4] == 1 and n[10 + 7] == 4


def test_frame_layer_without_stage_completion_on_two_queues(ctx):
    """Stage completion off; other work (uploads, a batch call) in flight on both queues; pictures of one geometry taken in
    turn on queues 0 and 1: the counts are per queue and the call waits for its own queue, so every result is complete
    and its own on return."""
    pics = [HC.FramePicture(ctx, np.int16, n & 1, 384, 288, 3, 1, seed=40 + n) for n in range(4)]
    filler = HC.mixed_specs(np.int16, seed=5)
    planes = [ctx.upload(s["buf"], stride=s["buf"].shape[1] * 2) for s in filler]
    # (a set of counts per queue: the batch call's counts are the caller's to keep apart)
    sets = [ctx.histogram_planes([(p, s["bands"]) for p, s in zip(planes, filler)]) for q in (0, 1)]
    try:
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 0))
        for rnd in range(2):
            for n, pic in enumerate(pics):
                other = (n + 1) & 1
                ctx.select_queue(other)
                sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, sets[other][0], len(filler), 2))  # left in flight on the other queue
                ctx.select_queue(n & 1)
                pic.check(unref=False)
        ctx.queue_synchronize(0)
        ctx.queue_synchronize(1)
    finally:
        ctx.select_queue(0)
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))
        ctx.synchronize()
    for (_, counts, _) in sets:
        for got, s in zip([c.download() for c in counts], filler):
            assert np.array_equal(got, HC.expected(s))
    for pic in pics:
        pic.iwt.unref()
    for p in planes + [sets[0][2], sets[1][2]]:
        p.free()


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_write_footprint(ctx, dtype):
    """The coefficient planes are unchanged byte for byte and nothing but the counts is written; the planes' padding and
    guards hold random bytes, so a count that depended on a sample outside its band -- row -1 of a DC band at the plane's
    first row among them -- would not equal the checker's."""
    b = np.dtype(dtype).itemsize
    specs = HC.mixed_specs(dtype, seed=29)
    L = G.Layout()
    regions = []
    for n, s in enumerate(specs):
        h, pitch = s["buf"].shape
        co = L.plane(h, pitch, dtype, align=256, skew=(2 * n * b) % 256, footprint=None, name="coeffs%d" % n)
        cn = L.span(420 * len(s["bands"]), align=4, footprint=("bytes", 420 * len(s["bands"])), name="counts%d" % n)
        regions.append((co, cn))
    B = G.GuardedBlock(ctx, L, seed=55)
    arr = (_lib.HistogramPlane * len(specs))()
    keep, want = [], {}
    for a, s, (co, cn) in zip(arr, specs, regions):
        B[co].upload(s["buf"])
        tab = (_lib.HistogramBand * len(s["bands"]))(*[_lib.HistogramBand(*bd) for bd in s["bands"]])
        keep.append(tab)
        a.coeffs, a.bytes, a.bands, a.nbands, a.counts = B[co].ptr, co.extent, tab, len(tab), B[cn].ptr
        want[co] = s["buf"]
        want[cn] = HC.expected(s).reshape(1, -1).view(np.uint8)
    sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, arr, len(specs), b))
    ctx.synchronize()
    B.check(want)
    B.free()


def test_byte_offsets_past_32_bits():
    """A band whose last row lies 4 GiB from its first sample (65 537 rows 65 536 bytes apart, 8 samples of every row
    counted): the row offset is 64-bit arithmetic -- in 32 bits the last row would be row 0 again.  Every sample is 257
    but the last row's, which are 1 .. 8.
    Needs 4 GiB + 64 KiB of device memory for a few milliseconds: a context of its own, closed at the end, so that the block
    goes back to the device with it instead of staying in the session context's allocation cache."""
    own = sa.Context(0)
    try:
        rows, pitch = 65537, 32768
        plane = own.plane(rows, pitch, np.int16, stride=2 * pitch).fill(1)
        last = np.arange(1, 9, dtype=np.int16).reshape(1, 8)
        sa.check(own.lib.schro_hip_upload_2d(own.h, plane.ptr + (rows - 1) * plane.stride, plane.stride, last.ctypes.data_as(C.c_void_p), 16, 16, 1))
        got, = own.histogram_batch([(plane, [(0, 2 * pitch, 8, rows, 1, 0), (0, 2 * pitch, 8, rows, 4, 0)])])
        plane.free()
    finally:
        own.close()
    for g, skip in zip(got, (1, 4)):
        want = np.zeros(105, np.uint32)
        want[int(H.ilogx(257))] = 8 * ((rows - 1) // skip)
        want[1:9] += 1
        assert np.array_equal(g, want), (skip, np.flatnonzero(g).tolist(), g[np.flatnonzero(g)].tolist())


def test_refusals_on_the_device(ctx):
    """every refusal, then the same planes taken: the context still works (the counts of a good call are right)"""
    assert HC.refusal_cases(ctx) >= 12
    x = all_s16()
    HC.run_specs(ctx, [dict(buf=x, bands=[HC.sub_band(x, 0, 0, 256, 256)])])
