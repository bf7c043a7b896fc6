"""GPU parity: the forward wavelet (schro_hip_iwt_batch, schro_hipframe_iwt_transform) vs the CPU oracle.

Every comparison is bit-exact (np.array_equal) against oracle_forward_iwt_component, which tests/test_oracle_wavelet.py
pins on the reference's compiled Orc kernels for filters 0 - 4 and 6.  Those filters are compared on pixel-range input,
where no intermediate wraps, and on full-range input, which exercises the wrap points.

The Fidelity filter (5) has no compiled reference kernel to be pinned on ("parity unpinned" stays for the inverse Fidelity
filter itself), but its FORWARD wrap points need none: filters 3 and 5, the two without a pre-shift, lift with wrap-around
additions only, so the inverse is a bijection and inverse (forward (x)) == x for every input, full range included
(tests/test_oracle_wavelet.py checks this of the oracle, and that it fails for the filters that lose the input's top
bit).  The device inverse of filter 5 is compared with the oracle's at full range (tests/test_gpu_iiwt.py), so the forward
transform of a full-range image is fixed as the one image that inverse maps back: the forward filter-5 comparison on
full-range input rests on the inverse, by the full-range round trip on the device below, not on reference output.

The round trip (forward on the device, then the existing inverse on the device, equals the input) is the design of the
reference's testsuite/wavelet_2d.c; the footprint cases use tests/guard_lib.py.
"""
import ctypes as C

import numpy as np
import pytest

import guard_lib as G
import oracle_lib as O
import schroedinger_amd as sa
import synth
from schroedinger_amd import frames

pytestmark = pytest.mark.gpu

FILTERS = range(7)
# (width, height): tiny, odd at a level (30 x 18: 15 x 9 sub-bands), one tile, several tiles, 1080p- and 2160p-sized
SIZES = [(2, 2), (4, 4), (8, 2), (16, 16), (30, 18), (256, 256), (320, 240), (1920, 1088), (3840, 2160)]


def pixel_range(h, w, dtype, seed):
    """-128 .. 127 (s16), -512 .. 511 (s32): what a transform of 8- / 10-bit pictures is fed."""
    v = synth.lcg(h * w, seed)
    if np.dtype(dtype) == np.int16:
        return ((v & 0xff).astype(np.int32) - 128).astype(np.int16).reshape(h, w)
    return ((v & 0x3ff).astype(np.int32) - 512).reshape(h, w)


def deepest(w, h, cap=4):
    d = 1
    while d < cap and w % (2 << d) == 0 and h % (2 << d) == 0:
        d += 1
    return d


def gpu_iwt(ctx, img, depth, filt):
    src = ctx.upload(img)
    dst = ctx.plane(img.shape[0], img.shape[1], img.dtype).fill(0x5a)
    ctx.iwt_batch([(src, dst)], depth, filt)
    out = dst.download()
    unchanged = src.download()
    src.free()
    dst.free()
    assert np.array_equal(unchanged, img), "the source plane was modified"
    return out


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", FILTERS)
def test_every_size_depth_and_range(ctx, filt, dtype):
    for (w, h) in SIZES:
        for depth in sorted({1, deepest(w, h)}):
            img = pixel_range(h, w, dtype, seed=w * 31 + h + depth)
            assert np.array_equal(gpu_iwt(ctx, img, depth, filt), O.forward_iwt(img, depth, filt)), (filt, w, h, depth, "pixel")
            # (filter 5 too: its full-range wrap points are fixed by the inverse's, see above)
            fr = synth.full_range(h, w, dtype, seed=w * 7 + h + depth)
            assert np.array_equal(gpu_iwt(ctx, fr, depth, filt), O.forward_iwt(fr, depth, filt)), (filt, w, h, depth, "full")


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", FILTERS)
def test_batch_of_unlike_planes(ctx, filt, dtype):
    # the components of a 4:2:0 and of a 4:2:2 picture and a 2 x 2 plane in ONE call (so one level), in both orders
    shapes = [(288, 352), (144, 176), (144, 176), (240, 320), (240, 160), (240, 160), (2, 2)]
    imgs = [pixel_range(h, w, dtype, seed=5 + n) for n, (h, w) in enumerate(shapes)]
    want = [O.forward_iwt(a, 1, filt) for a in imgs]
    for order in (list(range(len(imgs))), list(reversed(range(len(imgs))))):
        srcs = [ctx.upload(imgs[n]) for n in order]
        dsts = [ctx.plane(imgs[n].shape[0], imgs[n].shape[1], dtype).fill(0xa5) for n in order]
        ctx.iwt_batch(list(zip(srcs, dsts)), 1, filt)
        for k, n in enumerate(order):
            assert np.array_equal(dsts[k].download(), want[n]), (filt, shapes[n], order[0])
        [p.free() for p in srcs + dsts]
    # ... and the deeper levels of the pictures alone (the 2 x 2 plane has one level)
    srcs = [ctx.upload(a) for a in imgs[:6]]
    dsts = [ctx.plane(a.shape[0], a.shape[1], dtype).fill(0xa5) for a in imgs[:6]]
    ctx.iwt_batch(list(zip(srcs, dsts)), 4, filt)
    for n in range(6):
        assert np.array_equal(dsts[n].download(), O.forward_iwt(imgs[n], 4, filt)), (filt, shapes[n], "depth 4")
    [p.free() for p in srcs + dsts]


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", FILTERS)
def test_round_trip_is_the_identity(ctx, filt, dtype):
    for (w, h, depth) in [(320, 240, 4), (3840, 2160, 3)]:
        img = pixel_range(h, w, dtype, seed=17 + filt)
        src = ctx.upload(img)
        co = ctx.plane(h, w, dtype).fill(0x5a)
        back = ctx.plane(h, w, dtype).fill(0xa5)
        ctx.iwt_batch([(src, co)], depth, filt)
        ctx.iiwt_batch([(co, back)], depth, filt)
        got = back.download()
        [p.free() for p in (src, co, back)]
        assert np.array_equal(got, img), (filt, w, h, depth)


def round_trip(ctx, img, depth, filt):
    src = ctx.upload(img)
    co = ctx.plane(img.shape[0], img.shape[1], img.dtype).fill(0x5a)
    back = ctx.plane(img.shape[0], img.shape[1], img.dtype).fill(0xa5)
    ctx.iwt_batch([(src, co)], depth, filt)
    ctx.iiwt_batch([(co, back)], depth, filt)
    got_co, got = co.download(), back.download()
    [p.free() for p in (src, co, back)]
    return got_co, got


DEEP = [(64, 64, 6), (64, 128, 6), (32, 96, 5), (160, 96, 5)]      # (h, w, depth): last levels of 2 x 2 (1 x 2, 5 x 3 sub-bands)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", FILTERS)
def test_depths_5_and_6(ctx, filt, dtype):
    """The last levels read 4 x 4 and 2 x 2 images from the queue's scratch.  Pixel range: against the oracle, and the
    device round trip gives the input back; full range: against the oracle (every filter: the pinned ones and, by the
    argument at the top, filter 5), and the device inverse of the coefficients equals the oracle's inverse of them."""
    for (h, w, depth) in DEEP:
        img = pixel_range(h, w, dtype, seed=h * 13 + w + depth)
        co, back = round_trip(ctx, img, depth, filt)
        assert np.array_equal(co, O.forward_iwt(img, depth, filt)), (filt, w, h, depth, "pixel")
        assert np.array_equal(back, img), (filt, w, h, depth, "pixel round trip")
        fr = synth.full_range(h, w, dtype, seed=h * 5 + w + depth)
        co, back = round_trip(ctx, fr, depth, filt)
        want = O.forward_iwt(fr, depth, filt)
        assert np.array_equal(co, want), (filt, w, h, depth, "full")
        assert np.array_equal(back, O.inverse_iwt(want, depth, filt)), (filt, w, h, depth, "full inverse")
        if filt in (3, 5):
            assert np.array_equal(back, fr), (filt, w, h, depth, "full round trip")


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", [3, 5])
def test_full_range_round_trip_of_the_filters_without_a_pre_shift(ctx, filt, dtype):
    """forward, then inverse, on the device equals full-range input (the property tests/test_oracle_wavelet.py shows of the
    oracle): what the forward filter-5 comparison rests on."""
    for (h, w, depth) in [(36, 60, 2), (256, 256, 4), (64, 64, 6)]:
        fr = synth.full_range(h, w, dtype, seed=h + 3 * w + depth)
        co, back = round_trip(ctx, fr, depth, filt)
        assert np.array_equal(back, fr), (filt, w, h, depth)
        assert np.array_equal(co, O.forward_iwt(fr, depth, filt)), (filt, w, h, depth, "coefficients")


@pytest.mark.parametrize("filt", [1, 5])
def test_256_planes_in_one_call(ctx, filt):
    """The call's limit (the workgroup-to-job search goes round once per 64 jobs): 256 planes of mixed sizes from 2 x 2 to
    16 x 24, depth 1, every plane against the oracle, in both orders."""
    rng = np.random.default_rng(256 + filt)
    shapes = [(2, 2), (16, 24)] + [(2 * int(rng.integers(1, 9)), 2 * int(rng.integers(1, 13))) for _ in range(254)]
    imgs = [pixel_range(h, w, np.int16, seed=7 + n) for n, (h, w) in enumerate(shapes)]
    want = [O.forward_iwt(a, 1, filt) for a in imgs]
    srcs = [ctx.upload(a) for a in imgs]
    for order in (list(range(256)), list(range(256))[::-1]):
        dsts = [ctx.plane(shapes[n][0], shapes[n][1], np.int16).fill(0xa5) for n in order]
        ctx.iwt_batch([(srcs[n], d) for n, d in zip(order, dsts)], 1, filt)
        for n, d in zip(order, dsts):
            assert np.array_equal(d.download(), want[n]), (filt, n, shapes[n], order[0])
        [d.free() for d in dsts]
    [p.free() for p in srcs]


def run_guarded(ctx, planes, depth, filt, seed):
    """planes: (h, w, dtype, src stride, src (align, skew), dst stride, dst (align, skew)) -- one call, every plane of it in
    one guarded block: the payloads against the oracle, then every byte outside the dst rectangles against its canary
    (guards, row padding, the sources)."""
    L, todo = G.Layout(), []
    for n, (h, w, dt, ss, sl, ds, dl) in enumerate(planes):
        img = pixel_range(h, w, dt, seed + n)
        s = L.plane(h, w, dt, ss, *sl, footprint=None, name="src%d" % n)
        d = L.plane(h, w, dt, ds, *dl, footprint="rect", name="dst%d" % n)
        todo.append((s, d, img))
    B = G.GuardedBlock(ctx, L, seed)
    try:
        for s, _, img in todo:
            B[s].upload(img)
        ctx.iwt_batch([(B[s], B[d]) for s, d, _ in todo], depth, filt)
        ctx.synchronize()
        B.check({d: O.forward_iwt(img, depth, filt) for _, d, img in todo})
    finally:
        B.free()


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", FILTERS)
def test_footprint_small_unaligned_plane(ctx, filt, dtype):
    b = np.dtype(dtype).itemsize
    # sample-aligned leads, rows with an odd number of samples of padding: the element-wise loads and stores
    run_guarded(ctx, [(36, 60, dtype, 60 * b + 3 * b, (256, b), 60 * b + 5 * b, (256, 3 * b)),
                      (18, 30, dtype, 30 * b, (64, 8), 30 * b + b, (64, 16))], 1, filt, seed=3 + filt)
    # ... 8-byte loads, element-wise stores; two levels
    run_guarded(ctx, [(36, 60, dtype, 64 * b, (256, 0), 60 * b + 5 * b, (256, b))], 2, filt, seed=9 + filt)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", [0, 3, 5, 6])
def test_footprint_1080p_plane(ctx, filt, dtype):
    b = np.dtype(dtype).itemsize
    run_guarded(ctx, [(1080, 1920, dtype, 1920 * b + 64, (256, 0), 1920 * b + 128, (256, 0))], 3, filt, seed=21 + filt)


@pytest.mark.parametrize("case", [("420_s16", np.int16, 1, 1, 0, 3), ("422_s32", np.int32, 1, 0, 6, 4), ("444_s16", np.int16, 0, 0, 2, 3)],
                         ids=lambda c: c[0])
@pytest.mark.parametrize("complete", [1, 0])
def test_frame_layer(ctx, case, complete):
    _, dtype, hs, vs, filt, depth = case
    w, h = 320, 240
    planes = [pixel_range(h, w, dtype, 1), pixel_range(h >> vs, w >> hs, dtype, 2), pixel_range(h >> vs, w >> hs, dtype, 3)]
    params = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=w, iwt_luma_height=h,
                                iwt_chroma_width=w >> hs, iwt_chroma_height=h >> vs)
    fr = frames.DeviceFrame(ctx, frames.frame_format(dtype, hs, vs), w, h).upload(frames.HostFrame(planes, hs, vs))
    try:
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, complete))
        sa.check(ctx.lib.schro_hipframe_iwt_transform(ctx.h, fr.ptr(), C.byref(params)))
        # (twice in a row on one queue: the second call's copy into the scratch queues behind the first call's kernels)
        sa.check(ctx.lib.schro_hipframe_iwt_transform(ctx.h, fr.ptr(), C.byref(params)))
        ctx.synchronize()
    finally:
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))
    got = fr.download()
    fr.unref()
    for k in range(3):
        once = O.forward_iwt(planes[k], depth, filt)
        assert np.array_equal(got[k], O.forward_iwt(once, depth, filt)), (case[0], k)


@pytest.mark.parametrize("case", [("420_s16", np.int16, 1, 1, 0, 3), ("422_s32", np.int32, 1, 0, 6, 4)], ids=lambda c: c[0])
def test_frame_layer_equals_the_oracle_per_component(ctx, case):
    _, dtype, hs, vs, filt, depth = case
    w, h = 352, 288 if vs else 240
    planes = [pixel_range(h, w, dtype, 4), pixel_range(h >> vs, w >> hs, dtype, 5), pixel_range(h >> vs, w >> hs, dtype, 6)]
    params = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=w, iwt_luma_height=h,
                                iwt_chroma_width=w >> hs, iwt_chroma_height=h >> vs)
    fr = frames.DeviceFrame(ctx, frames.frame_format(dtype, hs, vs), w, h).upload(frames.HostFrame(planes, hs, vs))
    sa.check(ctx.lib.schro_hipframe_iwt_transform(ctx.h, fr.ptr(), C.byref(params)))
    got = fr.download()
    fr.unref()
    for k in range(3):
        assert np.array_equal(got[k], O.forward_iwt(planes[k], depth, filt)), (case[0], k)
