"""GPU parity: the encoder's quantisation (schro_hip_quantise_batch, schro_hipframe_quantise) and the frame subtract
(schro_hip_subtract_batch, schro_hipframe_subtract) against tests/quant_ref.py, bit for bit: quantised values,
reconstruction and codeblock summaries alike.  The checker is pinned on the reference's compiled Orc programs by
tests/test_quant_ref.py; its DC recurrence, which cannot be pinned that way, is held here against the product's decoder path
(schro_hip_dequant_batch + schro_hip_dc_predict_batch, themselves pinned on the reference decoder)."""
import ctypes as C

import numpy as np
import pytest

import guard_lib as G
import quant_cases as QC
import quant_ref as Q
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu


def test_every_value_every_index(ctx):
    """122 planes of 256 x 256 s16 holding all 65 536 values, one codeblock each, indices 0 .. 60 x inter / intra, one call."""
    x = Q.all_s16().reshape(256, 256)
    specs = [dict(buf=x, records=[[0, 512, 256, 256, qi]], intra=intra) for intra in (0, 1) for qi in range(61)]
    assert len(specs) == 122
    QC.run_specs(ctx, specs)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_codeblock_geometry(ctx, dtype):
    QC.run_specs(ctx, QC.geometry_specs(dtype, seed=11))


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_intra_ll_recurrence(ctx, dtype):
    specs = QC.dc_specs(dtype, seed=23, threads=sa.QUANTISE_DC_THREADS)
    QC.run_specs(ctx, specs)
    if dtype == np.int16:
        # the case is what it says: in the 65 x 64 band, stores of the recurrence truncated to 16 bits
        s = specs[4]
        Q.quantise_plane(s["buf"], s["records"], 1, s["dc"][0], s["dc"][1:])
        assert Q.quantise_dc.truncated > 0


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("intra", [0, 1])
def test_round_trip_through_the_decoder_path(ctx, dtype, intra):
    """quantise, then the product's decoder: schro_hip_dequant_batch (arith 0) on the quantised values, for intra
    schro_hip_dc_predict_batch on the LL band -- equals the encoder's in-place reconstruction (|x| <= 4095)."""
    rng = np.random.default_rng(5 + intra)
    b = np.dtype(dtype).itemsize
    w, h, depth, pitch = 80, 48, 2, 83
    recs = QC.layout(w, h, depth, [2, 2, 3], [2, 1, 2], pitch * b, b)
    for n, r in enumerate(recs):
        r[4] = (0, 3, 4, 7, 12, 17, 22, 31, 50, 60)[n % 10]
    buf = rng.integers(-4095, 4096, (h, pitch)).astype(dtype)
    spec = dict(buf=buf, records=recs, intra=intra, dc=(4, w >> depth, h >> depth) if intra else None)
    (q, r), = QC.run_specs(ctx, [spec])
    blob, drecs = QC.tight_values(q, recs, b)
    dst = ctx.plane(h, pitch, dtype, stride=pitch * b).fill(0x33)
    vals = ctx.upload_bytes(blob)
    ctx.dequant_batch([(dst, vals, drecs, intra)], arith=0)
    if intra:
        ctx.dc_predict_batch([_ll_view(dst, w, depth)])
    got = dst.download()
    mask = QC.record_mask(buf.shape, recs, b)
    assert np.array_equal(got[mask], r[mask])
    dst.free()
    vals.free()


def _ll_view(plane, w, depth):
    v = plane.level_view(depth)
    v.width = w >> depth        # (the plane's rows carry padding samples: the band is the transform's, not the pitch's)
    return v


class FramePicture:
    """One 4:2:0 picture for schro_hipframe_quantise: its device frames, records, quant indices and host summaries (pinned:
    with stage completion off the copy back stays asynchronous), and what tests/quant_ref.py expects of the call."""

    def __init__(self, ctx, dtype, intra, w, h, depth, hc, vc, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.dtype, self.intra, self.size, self.depth, self.hc, self.vc = ctx, dtype, intra, (w, h), depth, hc, vc
        b = np.dtype(dtype).itemsize
        self.planes = [QC.values(rng, (h, w), dtype), QC.values(rng, (h // 2, w // 2), dtype), QC.values(rng, (h // 2, w // 2), dtype)]
        fmt = frames.frame_format(dtype, 1, 1)
        self.iwt = frames.DeviceFrame(ctx, fmt, w, h).upload(frames.HostFrame(self.planes, 1, 1))
        self.quant = frames.DeviceFrame(ctx, fmt, w, h)
        self.params = frames.make_params(transform_depth=depth, num_refs=0 if intra else 1, iwt_luma_width=w, iwt_luma_height=h,
                                         iwt_chroma_width=w // 2, iwt_chroma_height=h // 2)
        for l in range(depth + 1):
            self.params.horiz_codeblocks[l], self.params.vert_codeblocks[l] = hc[l], vc[l]
        self.recs, self.idx, self.summ = [], [], []
        for k in range(3):
            cw, ch = (w, h) if k == 0 else (w // 2, h // 2)
            r = QC.layout(cw, ch, depth, hc, vc, self.iwt.c.components[k].stride, b)
            for n, rec in enumerate(r):
                rec[4] = (5 * n + 7 * k + seed) % 61
            self.recs.append(r)
            self.idx.append((C.c_int * len(r))(*[rec[4] for rec in r]))
            self.summ.append(ctx.host_array((len(r), 2), np.uint32))
            self.summ[-1][:] = 0xdeadbeef

    def issue(self):
        qi = (C.POINTER(C.c_int) * 3)(*[C.cast(a, C.POINTER(C.c_int)) for a in self.idx])
        sp = (C.POINTER(_lib.CodeblockSummary) * 3)(*[C.cast(a.ctypes.data, C.POINTER(_lib.CodeblockSummary)) for a in self.summ])
        sa.check(self.ctx.lib.schro_hipframe_quantise(self.quant.ptr(), self.iwt.ptr(), C.byref(self.params), qi, sp))

    def check(self):
        """(after the queue has been waited for)"""
        (w, h), b, depth = self.size, np.dtype(self.dtype).itemsize, self.depth
        got_r, got_q = self.iwt.download(), self.quant.download()
        for k in range(3):
            cw, ch = (w, h) if k == 0 else (w // 2, h // 2)
            pitch = self.iwt.c.components[k].stride // b
            buf = np.zeros((ch, pitch), self.dtype)
            buf[:, :cw] = self.planes[k]
            dc = (self.hc[0] * self.vc[0], cw >> depth, ch >> depth) if self.intra else None
            want_q, want_r, want_s = Q.quantise_plane(buf, self.recs[k], self.intra, dc[0] if dc else 0, dc[1:] if dc else None)
            assert np.array_equal(got_q[k], want_q[:, :cw]), (k, "quantised values")
            assert np.array_equal(got_r[k], want_r[:, :cw]), (k, "reconstruction")
            assert self.summ[k].tolist() == [list(s) for s in want_s], (k, "summaries")
        self.iwt.unref()
        self.quant.unref()


def frame_case(ctx, dtype, intra, w, h, depth, hc, vc, seed):
    """schro_hipframe_quantise on a 4:2:0 picture against the batch call's checker"""
    pic = FramePicture(ctx, dtype, intra, w, h, depth, hc, vc, seed)
    pic.issue()
    ctx.synchronize()           # (with stage completion off the summaries are complete only now)
    pic.check()


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("intra", [0, 1])
def test_frame_layer_quantise(ctx, dtype, intra):
    frame_case(ctx, dtype, intra, 64, 48, 2, [1, 2, 3], [1, 2, 2], seed=3)
    # another geometry on the same context: the table of records and summaries is rebuilt ...
    frame_case(ctx, dtype, intra, 64, 48, 2, [2, 1, 4], [1, 1, 3], seed=4)
    # ... and the first one again
    frame_case(ctx, dtype, intra, 64, 48, 2, [1, 2, 3], [1, 2, 2], seed=5)


def test_frame_layer_quantise_without_stage_completion(ctx):
    try:
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 0))
        frame_case(ctx, np.int16, 1, 64, 48, 2, [1, 2, 3], [1, 2, 2], seed=8)
    finally:
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_frame_layer_quantise_pictures_in_flight_on_two_queues(ctx, dtype):
    """Stage completion off, pictures of ONE geometry enqueued in turn on queues 0 and 1 and not ordered against each
    other: the device summaries are per queue, so every picture's zero counts and maxima are its own.  The pictures are
    large enough (a few hundred workgroups, a DC band of 95 diagonals) for a call's kernels to be in flight while the next
    call's clear and kernels are enqueued on the other queue; several rounds reuse each queue's summaries."""
    geo = (384, 288, 3, [1, 1, 2, 3], [1, 1, 2, 2])
    pics = [FramePicture(ctx, dtype, 1, *geo, seed=20 + n) for n in range(6)]
    try:
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 0))
        for n, pic in enumerate(pics):
            ctx.select_queue(n & 1)
            pic.issue()
        ctx.queue_synchronize(0)
        ctx.queue_synchronize(1)
    finally:
        ctx.select_queue(0)
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))
        ctx.synchronize()
    for pic in pics:
        pic.check()


@pytest.mark.parametrize("src_dtype", [np.int16, np.uint8])
def test_subtract_batch_and_frame_layer(ctx, src_dtype):
    rng = np.random.default_rng(41)

    def src_plane(h, w):
        return (rng.integers(0, 256, (h, w)) if src_dtype == np.uint8 else rng.integers(-32768, 32768, (h, w))).astype(src_dtype)
    # planes: odd sizes, a source smaller and larger than the destination
    cases = [((37, 61), (37, 61)), ((40, 70), (33, 90)), ((1, 1), (1, 1)), ((19, 200), (25, 131))]
    pairs, want = [], []
    for (dh, dw), (sh, sw) in cases:
        d, s = rng.integers(-32768, 32768, (dh, dw)).astype(np.int16), src_plane(sh, sw)
        pairs.append((ctx.upload(d, stride=dw * 2 + 6), ctx.upload(s, stride=sw * s.itemsize + 3 * s.itemsize)))
        want.append(Q.subtract(d, s))
    ctx.subtract_batch(pairs)
    for (d, s), w_ in zip(pairs, want):
        assert np.array_equal(d.download(), w_)
        d.free()
        s.free()
    # frames: 4:2:0, the source frame smaller than the destination -- the common size of each component
    dp = [rng.integers(-32768, 32768, s).astype(np.int16) for s in ((48, 64), (24, 32), (24, 32))]
    sp = [src_plane(*s) for s in ((40, 60), (20, 30), (20, 30))]
    dest = frames.DeviceFrame(ctx, frames.frame_format(np.int16, 1, 1), 64, 48).upload(frames.HostFrame(dp, 1, 1))
    src = frames.DeviceFrame(ctx, frames.frame_format(src_dtype, 1, 1), 60, 40).upload(frames.HostFrame(sp, 1, 1))
    sa.check(ctx.lib.schro_hipframe_subtract(dest.ptr(), src.ptr()))
    got = dest.download()
    for k in range(3):
        assert np.array_equal(got[k], Q.subtract(dp[k], sp[k])), k
    # any other pair of formats is refused
    s32 = frames.DeviceFrame(ctx, frames.frame_format(np.int32, 1, 1), 64, 48)
    s422 = frames.DeviceFrame(ctx, frames.frame_format(np.int16, 1, 0), 64, 48)
    for a, b_ in ((s32, src), (dest, s32), (dest, s422), (src, dest) if src_dtype == np.uint8 else (s32, dest)):
        assert ctx.lib.schro_hipframe_subtract(a.ptr(), b_.ptr()) == QC.EINVAL
        assert b"hipframe_subtract" in ctx.lib.schro_hip_last_error()
    for f in (dest, src, s32, s422):
        f.unref()


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_write_footprint(ctx, dtype):
    """Nothing outside the records' rectangles is written in either plane -- the gap between a band's width and its stride
    included --, and the summary buffer gets exactly ncodeblocks entries."""
    b = np.dtype(dtype).itemsize
    specs = QC.geometry_specs(dtype, seed=17)[:4] + QC.dc_specs(dtype, seed=19, threads=8)[3:5]
    L = G.Layout()
    regions = []
    for n, s in enumerate(specs):
        h, pitch = s["buf"].shape
        fp = [(r[0], r[1], r[2] * b, r[3]) for r in s["records"]]
        co = L.plane(h, pitch, dtype, align=256, skew=(2 * n * b) % 256, footprint=fp, name="coeffs%d" % n)
        qu = L.plane(h, pitch, dtype, align=64, skew=b, footprint=fp, name="quant%d" % n)
        su = L.span(8 * len(s["records"]), align=8, footprint=("bytes", 8 * len(s["records"])), name="summary%d" % n)
        regions.append((co, qu, su))
    B = G.GuardedBlock(ctx, L, seed=77)
    arr = (_lib.QuantPlane * len(specs))()
    keep, want = [], {}
    for a, s, (co, qu, su) in zip(arr, specs, regions):
        B[co].upload(s["buf"])
        tab = QC.table(s["records"])
        keep.append(tab)
        a.coeffs, a.quant, a.bytes = B[co].ptr, B[qu].ptr, co.extent
        a.codeblocks, a.ncodeblocks, a.is_intra, a.summary = tab, len(tab), s["intra"], B[su].ptr
        if s.get("dc"):
            a.dc_predict_first, a.dc_width, a.dc_height = s["dc"]
        q, r, summ = Q.quantise_plane(s["buf"], s["records"], s["intra"], s["dc"][0] if s.get("dc") else 0,
                                      s["dc"][1:] if s.get("dc") else None)
        mask = QC.record_mask(s["buf"].shape, s["records"], b)
        want[co] = r
        want[qu] = np.where(mask, q, B[qu].initial())
        want[su] = np.array(summ, np.uint32).reshape(1, -1).view(np.uint8)
    sa.check(ctx.lib.schro_hip_quantise_batch(ctx.h, arr, len(specs), b))
    ctx.synchronize()
    B.check(want)
    B.free()


def test_refusals_on_the_device(ctx):
    assert QC.refusal_cases(ctx) >= 10
