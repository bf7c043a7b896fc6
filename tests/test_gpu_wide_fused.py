"""GPU: v216 / ARGB / AY64 written by the finest wavelet level (iiwt.hip, iiwt_wide_kernel) -- schro_hip_iiwt_pack_wide_batch.

The non-reference intra tail of a > 8-bit picture: the inverse wavelet, schro_frame_shift_right, the packed copy-out.  The
LEVEL route does it without the pixel frame: levels depth-1 .. 1 by the level loop, then ONE launch per kernel family that
lifts the finest level of Y, U and V per tile, shifts, converts and writes whole 16-byte groups.  Every case is compared
bit for bit with the oracle's chain

    O.pack_wide ([O.shift_right (O.inverse_iwt (c, depth, filt)[:oh, :cw], shift) ...], hs, 0, ow, oh, fmt)

must report its route, launch nothing of the "convert" profile class on LEVEL, and leave every byte outside the packed rows
as it was: coefficient planes and dst are carved out of a guarded block (tests/guard_lib.py), dst three rows and 32 bytes
per row larger than the packed rows and sentinel-filled.  Half of the pictures of a call carry full-range coefficients
(+- 2^19 cast to the sample type: the s32 -> s16 truncation, the 16-bit wrap points of the shift, AY64's clamp, ARGB's
modulo-256 bytes), half are forward-transformed pictures."""
import ctypes as C
import os

import numpy as np
import pytest

import guard_lib as G
import oracle_lib as O
import schroedinger_amd as sa
import synth
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a
EINVAL = -1             # SCHRO_HIP_EINVAL (include/schro_hip.h)
V216, ARGB, AY64 = sa.FORMAT_V216, sa.FORMAT_ARGB, sa.FORMAT_AY64
FORMATS = [(V216, 1), (ARGB, 0), (AY64, 0)]             # (format, its own h_shift; v_shift is 0)
FORMAT_IDS = ["422-v216", "444-argb", "444-ay64"]
NAMES = {V216: "v216", ARGB: "argb", AY64: "ay64"}

# Which format x sample type x filter takes LEVEL in the product library: exactly where scripts/wide_fused_ab.py measured LEVEL
# faster than the chain by more than the larger of the two forms' spreads, without a shift AND with one
# (profiles/r10_wide_fused.txt; wide_level_combination, iiwt_pack.cpp).  Everything else keeps the two passes.
# tests/test_gpu_wide_experiments.py runs this file again on the experiments library with SCHRO_HIP_WIDE_LEVEL=1 (every
# combination on LEVEL) and with SCHRO_HIP_WIDE_TWO_PASS=1 (every picture on the two passes).
LEVEL_FILTERS = {
    ("v216", 2): (0, 1, 2, 3, 4, 5, 6), ("v216", 4): (0, 1, 2, 3, 4, 5, 6),
    ("argb", 2): (0, 1, 3, 4), ("argb", 4): (0, 1, 2, 3, 4, 5, 6),
    ("ay64", 2): (0, 1, 2, 3, 4, 5), ("ay64", 4): (0, 1, 2, 3, 4, 5, 6),
}
_EXP = "exp" in os.path.basename(os.environ.get("SCHRO_HIP_LIB", ""))
FORCED_LEVEL = _EXP and os.environ.get("SCHRO_HIP_WIDE_LEVEL") == "1"
FORCED_TWO_PASS = _EXP and os.environ.get("SCHRO_HIP_WIDE_TWO_PASS") == "1"


def native_route(fmt, filt, dtype):
    """The route of a picture aligned as the level kernel asks."""
    if FORCED_TWO_PASS:
        return "two_pass"
    return "level" if FORCED_LEVEL or filt in LEVEL_FILTERS[(NAMES[fmt], np.dtype(dtype).itemsize)] else "two_pass"


def coefficients(w, h, hs, dtype, depth, filt, seed, full):
    dims = [(h, w), (h, w >> hs), (h, w >> hs)]
    if full:
        rng = np.random.default_rng(seed)
        return [rng.integers(-(1 << 19), 1 << 19, size=d).astype(np.int64).astype(dtype) for d in dims]
    return [O.forward_iwt((synth.image_s(a, b, dtype, seed=seed + k).astype(np.int64) * 37).astype(dtype), depth, filt)
            for k, (a, b) in enumerate(dims)]


def oracle_bytes(co, depth, filt, hs, ow, oh, fmt, shift):
    planes = []
    for k, c in enumerate(co):
        cw = ow if k == 0 else (ow + hs) >> hs
        planes.append(O.shift_right(O.inverse_iwt(c, depth, filt)[:oh, :cw], shift))
    return O.pack_wide(planes, hs, 0, ow, oh, fmt)


def run(ctx, pictures, depth, filt, dtype, route="level"):
    """pictures: dicts {w, h, ow, oh, fmt, hs, full, shift, + optional dst_pad (extra bytes of dst stride), route} -- one call."""
    lay, specs = G.Layout(), []
    for n, p in enumerate(pictures):
        w, h, hs = p["w"], p["h"], p["hs"]
        row = G.packed_row_bytes(p["fmt"], p["ow"])
        cs = [lay.plane(h, w if k == 0 else w >> hs, dtype, footprint=None, name="coeff%d.%d" % (n, k)) for k in range(3)]
        stride = -(-(row + 32) // 16) * 16 + p.get("dst_pad", 0)
        d = lay.plane(p["oh"] + 3, row + 32, np.uint8, stride=stride, footprint=[(0, stride, row, p["oh"])], name="dst%d" % n)
        specs.append((cs, d, row))
    blk = G.GuardedBlock(ctx, lay, seed=100 * filt + depth)
    jobs, expected, want_routes = [], {}, {"level": 0, "two_pass": 0}
    for n, (p, (cs, d, row)) in enumerate(zip(pictures, specs)):
        seed = 1000 * filt + 100 * depth + 10 * n + (p["fmt"] & 7)
        co = coefficients(p["w"], p["h"], p["hs"], dtype, depth, filt, seed, p["full"])
        for s, c in zip(cs, co):
            blk[s].upload(c)
        want = oracle_bytes(co, depth, filt, p["hs"], p["ow"], p["oh"], p["fmt"], p["shift"])
        if p["full"] and p["fmt"] == AY64 and np.dtype(dtype).itemsize == 4 and p["shift"] <= 2:
            words = want.view("<u2")
            assert words.min() == 0 and words.max() == 0xffff, ("the full-range case does not reach both ends of the clamp", n)
        full = np.full((p["oh"] + 3, row + 32), SENTINEL, np.uint8)
        blk[d].upload(full)
        full[:p["oh"], :row] = want
        expected[d] = full
        jobs.append(([blk[s] for s in cs], p["hs"], 0, blk[d], p["ow"], p["oh"], p["fmt"], p["shift"]))
        r = p.get("route", route)
        want_routes[native_route(p["fmt"], filt, dtype) if r == "level" else r] += 1
    ctx.synchronize()
    ctx.wide_routes(reset=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        ctx.iiwt_pack_wide_batch(jobs, depth, filt)
        ctx.synchronize()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    routes = ctx.wide_routes(reset=True)
    case = (depth, filt, np.dtype(dtype).name, [(NAMES[p["fmt"]], p["shift"]) for p in pictures])
    try:
        assert routes == want_routes, (case, routes, want_routes)
        if not want_routes["two_pass"]:
            assert prof["convert"][1] == 0, (case, prof["convert"])
        blk.check(expected)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (case, e))
    finally:
        blk.free()


def batch(depth, fmt, hs, shifts):
    """Unlike pictures in one call (luma sizes multiples of 2^(depth+1)): one tile; several tiles across and down with partial
    last ones, an out_width that ends in a partial group of every format (165 pairs, 331 pixels) inside a wider transform; a
    whole number of groups; a second cropped one (75 pairs, 150 pixels); and (depths 1, 2) chroma bands whose sub-band rows are
    no whole 8-byte vectors.  Alternately full-range and transformed; the shifts go round."""
    sizes = [(64, 32, 64, 32), (352, 160, 331, 150), (256, 96, 256, 96), (160, 64, 150, 62)]
    if depth == 1:
        sizes.append((44, 12, 41, 11))
    if depth == 2:
        sizes.append((40, 12, 40, 9))
    return [dict(w=w, h=h, ow=ow, oh=oh, fmt=fmt, hs=hs, full=n % 2 == 0, shift=shifts[n % len(shifts)])
            for n, (w, h, ow, oh) in enumerate(sizes)]


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("fmt,hs", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("filt", range(7))
def test_every_format_filter_depth_and_sample_type(ctx, filt, depth, fmt, hs, dtype):
    run(ctx, batch(depth, fmt, hs, (2, 0, 2, 2, 0)), depth, filt, dtype)       # (every picture kind with the shift and without)
    run(ctx, batch(depth, fmt, hs, (0, 2, 0, 0, 2)), depth, filt, dtype)


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("fmt,hs", FORMATS, ids=FORMAT_IDS)
def test_the_largest_shift(ctx, fmt, hs, dtype):
    top = 8 * np.dtype(dtype).itemsize - 1
    for filt in (0, 3):
        run(ctx, batch(3, fmt, hs, (top,)), 3, filt, dtype)


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("fmt,hs", FORMATS, ids=FORMAT_IDS)
def test_1080_rows_inside_a_1088_row_transform(ctx, fmt, hs, dtype):
    for filt in (1, 5):
        run(ctx, [dict(w=384, h=1088, ow=384, oh=1080, fmt=fmt, hs=hs, full=False, shift=2)], 4, filt, dtype)


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("depth", [1, 3])
def test_formats_and_routes_mixed_in_one_call(ctx, depth, dtype):
    """v216 + ARGB + AY64, with and without a shift; pictures the level kernel cannot take (a dst stride of 8 mod 16) beside
    pictures it can: each must give the oracle's bytes, so both routes give the same."""
    for filt in (0, 4):
        pics = []
        for n, (fmt, hs) in enumerate(FORMATS + FORMATS):
            two = n >= 3
            pics.append(dict(w=352, h=160, ow=331, oh=150, fmt=fmt, hs=hs, full=n % 2 == 1, shift=(0, 3, 1)[n % 3],
                             route="two_pass" if two else "level", dst_pad=8 if two else 0))
        run(ctx, pics, depth, filt, dtype)


class View:
    """width x height samples of `dtype` at byte `offset` of a device allocation."""

    def __init__(self, ctx, base, offset, height, width, dtype, stride):
        self.ctx, self.ptr, self.height, self.width, self.dtype, self.stride = ctx, base + offset, height, width, np.dtype(dtype), stride

    def upload(self, a):
        a = np.ascontiguousarray(a, self.dtype)
        sa.check(self.ctx.lib.schro_hip_upload_2d(self.ctx.h, self.ptr, self.stride, a.ctypes.data_as(C.c_void_p), a.strides[0],
                                                  self.width * self.dtype.itemsize, self.height))
        return self

    def download(self):
        out = np.empty((self.height, self.width), self.dtype)
        sa.check(self.ctx.lib.schro_hip_download_2d(self.ctx.h, out.ctypes.data_as(C.c_void_p), out.strides[0], self.ptr, self.stride,
                                                    self.width * self.dtype.itemsize, self.height))
        return out


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("fmt,hs", FORMATS, ids=FORMAT_IDS)
def test_a_dst_that_overlaps_a_coefficient_plane_takes_the_two_passes(ctx, fmt, hs, dtype):
    """dst begins inside the picture's own V coefficient plane: the two passes read every coefficient before the pack writes.
    A second picture of the same call, with planes of its own, takes LEVEL; both give the oracle's bytes."""
    w, h, ow, oh, depth, filt, shift = 160, 64, 150, 62, 2, 1, 1
    bpp = np.dtype(dtype).itemsize
    co = coefficients(w, h, hs, dtype, depth, filt, 77, False)
    want = oracle_bytes(co, depth, filt, hs, ow, oh, fmt, shift)
    row = want.shape[1]
    stride = -(-row // 16) * 16
    cw = w >> hs
    v_bytes = cw * bpp * h
    d_co = [ctx.upload(c) for c in co]                            # (the second picture's)
    d_y, d_u = ctx.upload(co[0]), ctx.upload(co[1])
    n = v_bytes + stride * oh + 4096
    base = ctx.alloc(n)
    whole = View(ctx, base, 0, 1, n, np.uint8, n).upload(np.full((1, n), SENTINEL, np.uint8))
    d_v = View(ctx, base, 0, h, cw, dtype, cw * bpp).upload(co[2])
    at = (v_bytes - 3 * cw * bpp) // 256 * 256                 # 16-byte aligned, inside V's last rows
    d_over = View(ctx, base, at, oh, row, np.uint8, stride)
    d_own = ctx.plane(oh, row, np.uint8, stride=stride).fill(SENTINEL)
    ctx.synchronize()
    ctx.wide_routes(reset=True)
    ctx.iiwt_pack_wide_batch([([d_y, d_u, d_v], hs, 0, d_over, ow, oh, fmt, shift), (d_co, hs, 0, d_own, ow, oh, fmt, shift)], depth, filt)
    ctx.synchronize()
    want_routes = {"level": 0, "two_pass": 1}
    want_routes[native_route(fmt, filt, dtype)] += 1
    assert ctx.wide_routes(reset=True) == want_routes
    assert np.array_equal(d_over.download(), want)
    assert np.array_equal(d_own.download(), want)
    raw = whole.download()[0]
    mask = np.zeros(n, bool)
    for y in range(oh):
        mask[at + y * stride:at + y * stride + row] = True
    before = np.full(n, SENTINEL, np.uint8)
    before[:v_bytes] = np.ascontiguousarray(co[2]).view(np.uint8).reshape(-1)
    assert np.array_equal(raw[~mask], before[~mask]), "bytes outside the packed rows changed"
    ctx.free(base)
    [p.free() for p in d_co + [d_y, d_u, d_own]]


def test_unaligned_coefficient_planes_take_the_two_passes(ctx):
    # a coefficient stride that is no multiple of the sample size cannot be expressed; a plane one byte off its sample size can
    w, h, ow, oh, depth, filt = 64, 32, 64, 32, 2, 3
    for fmt, hs in FORMATS:
        co = coefficients(w, h, hs, np.int32, depth, filt, 5, True)
        want = oracle_bytes(co, depth, filt, hs, ow, oh, fmt, 2)
        n = w * 4 * h + 64
        base = ctx.alloc(n)
        d_y = View(ctx, base, 2, h, w, np.int32, w * 4).upload(co[0])           # 2 mod 4
        d_u, d_v = ctx.upload(co[1]), ctx.upload(co[2])
        dst = ctx.plane(oh, want.shape[1], np.uint8).fill(SENTINEL)
        ctx.wide_routes(reset=True)
        ctx.iiwt_pack_wide_batch([([d_y, d_u, d_v], hs, 0, dst, ow, oh, fmt, 2)], depth, filt)
        ctx.synchronize()
        assert ctx.wide_routes(reset=True) == {"level": 0, "two_pass": 1}
        assert np.array_equal(dst.download(), want), NAMES[fmt]
        ctx.free(base)
        [p.free() for p in (d_u, d_v, dst)]


def test_refusals_launch_and_count_nothing(ctx):
    co = [ctx.upload(np.zeros(d, np.int16)) for d in [(32, 64), (32, 32), (32, 32)]]
    co444 = [ctx.upload(np.zeros((32, 64), np.int16)) for _ in range(3)]
    dst = ctx.plane(32, 512, np.uint8).fill(SENTINEL)
    ctx.synchronize()
    ctx.wide_routes(reset=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        arr = (_lib.IwtPackWidePicture * 2)()

        def fill(a, planes, hs, fmt):
            for k in range(3):
                a.src[k], a.src_stride[k] = planes[k].ptr, planes[k].stride
            a.width, a.height, a.h_shift, a.v_shift = 64, 32, hs, 0
            a.dst, a.dst_stride, a.out_width, a.out_height, a.format, a.shift = dst.ptr, dst.stride, 64, 32, fmt, 0

        call = lambda n=1, depth=3, bps=2: ctx.lib.schro_hip_iiwt_pack_wide_batch(ctx.h, arr, n, depth, 3, bps)
        a = arr[0]
        fill(a, co, 1, V216)
        assert call() == 0
        ctx.synchronize()
        good_prof = ctx.profile_read()          # (the launches of the one good call: the refused calls add none)
        good_routes = ctx.wide_routes()
        dst.fill(SENTINEL)
        ctx.synchronize()
        ctx.profile_reset()
        bad = 0
        for field, value in [("format", sa.FORMAT_V210), ("format", sa.FORMAT_AYUV), ("h_shift", 0), ("v_shift", 1), ("out_width", 66),
                             ("out_height", 33), ("out_width", 0), ("dst_stride", 8 * 32 - 1), ("shift", -1), ("shift", 16)]:
            keep = getattr(a, field)
            setattr(a, field, value)
            assert call() == EINVAL, (field, value)
            setattr(a, field, keep)
            bad += 1
        assert call(depth=6) == EINVAL                                     # 64 x 32 is not a multiple of 2^6
        assert call(bps=3) == EINVAL                                       # bytes_per_sample
        a.shift = 31
        assert call(bps=2) == EINVAL                                       # legal for s32 only
        a.shift = 0
        a.src_stride[1] = 62                                               # shorter than a chroma row
        assert call() == EINVAL
        a.src_stride[1] = co[1].stride
        # the 4:4:4 formats refuse a 4:2:2 source and a stride below their packed rows
        for fmt, rowb in ((ARGB, 4 * 64), (AY64, 8 * 64)):
            fill(a, co444, 1, fmt)
            assert call() == EINVAL, NAMES[fmt]
            fill(a, co444, 0, fmt)
            a.dst_stride = rowb - 1
            assert call() == EINVAL, NAMES[fmt]
        # a good picture in front of a bad one in the same call: nothing launched, nothing counted
        fill(arr[0], co, 1, V216)
        fill(arr[1], co, 1, V216)
        arr[1].shift = 16
        assert call(n=2) == EINVAL
        ctx.synchronize()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    assert ctx.wide_routes(reset=True) == good_routes and sum(good_routes.values()) == 1
    assert all(v[1] == 0 for v in prof.values()), prof
    assert any(v[1] for v in good_prof.values())
    assert (dst.download() == SENTINEL).all()
    [p.free() for p in co + co444 + [dst]]


# ---- the frame layer ------------------------------------------------------------------------------------------------

def up(v, depth):
    return -(-v // (1 << depth)) * (1 << depth)


def frame_case(ctx, fmt, hs, dtype, w=320, h=240, depth=3, filt=1):
    iw = [(up(h, depth), up(w, depth)), (up(h, depth), up(w, depth) >> hs), (up(h, depth), up(w, depth) >> hs)]
    params = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=iw[0][1], iwt_luma_height=iw[0][0],
                                iwt_chroma_width=iw[1][1], iwt_chroma_height=iw[1][0], num_refs=0)
    coeffs = [O.forward_iwt((synth.image_s(ih, iwd, dtype, seed=20 + k).astype(np.int64) * 37).astype(dtype), depth, filt)
              for k, (ih, iwd) in enumerate(iw)]
    fmt_t = frames.frame_format(dtype, hs, 0)
    dev_tf = frames.DeviceFrame(ctx, fmt_t, iw[0][1], iw[0][0]).upload(frames.HostFrame(coeffs, hs, 0))
    return params, coeffs, fmt_t, dev_tf, iw


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("fmt,hs", FORMATS, ids=FORMAT_IDS)
def test_frame_layer_convert_and_shift_convert(ctx, fmt, hs, dtype):
    """schro_frame_inverse_iwt_transform_convert_hip into a v216 / ARGB / AY64 frame = schro_frame_inverse_iwt_transform_hip +
    schro_hipframe_convert = the oracle; _shift_convert_hip = transform + schro_hipframe_shift_right + convert = the oracle."""
    w, h, depth, filt = 320, 240, 3, 1
    lib = ctx.lib
    params, coeffs, fmt_t, dev_tf, iw = frame_case(ctx, fmt, hs, dtype, w, h, depth, filt)
    row = G.packed_row_bytes(fmt, w)
    for shift in (0, 2, 8 * np.dtype(dtype).itemsize - 1):
        pixel = frames.DeviceFrame(ctx, fmt_t, iw[0][1], iw[0][0])
        want, got = frames.DeviceFrame(ctx, fmt, w, h), frames.DeviceFrame(ctx, fmt, w, h)
        sa.check(lib.schro_frame_inverse_iwt_transform_hip(pixel.ptr(), dev_tf.ptr(), C.byref(params)))
        if shift:
            sa.check(lib.schro_hipframe_shift_right(pixel.ptr(), shift))
        sa.check(lib.schro_hipframe_convert(want.ptr(), pixel.ptr()))
        ctx.wide_routes(reset=True)
        if shift == 0:
            sa.check(lib.schro_frame_inverse_iwt_transform_convert_hip(got.ptr(), dev_tf.ptr(), C.byref(params)))
        else:
            sa.check(lib.schro_frame_inverse_iwt_transform_shift_convert_hip(got.ptr(), dev_tf.ptr(), C.byref(params), shift))
        level = native_route(fmt, filt, dtype) == "level"
        assert ctx.wide_routes(reset=True) == {"level": int(level), "two_pass": int(not level)}
        g = np.asarray(got.download()).reshape(h, -1)[:, :row]
        assert np.array_equal(g, np.asarray(want.download()).reshape(h, -1)[:, :row]), shift
        assert np.array_equal(g, oracle_bytes(coeffs, depth, filt, hs, w, h, fmt, shift)), shift
        if shift == 0:
            # shift 0 through the new call is the same picture
            again = frames.DeviceFrame(ctx, fmt, w, h)
            sa.check(lib.schro_frame_inverse_iwt_transform_shift_convert_hip(again.ptr(), dev_tf.ptr(), C.byref(params), 0))
            assert np.array_equal(np.asarray(again.download()).reshape(h, -1)[:, :row], g)
            again.unref()
        for f in (pixel, want, got):
            f.unref()
    dev_tf.unref()


def test_frame_layer_refusals(ctx):
    lib = ctx.lib
    w, h = 320, 240
    # a prediction with a wide format
    for fmt, hs in FORMATS:
        params, _, _, dev_tf, _ = frame_case(ctx, fmt, hs, np.int16)
        packed = frames.DeviceFrame(ctx, fmt, w, h)
        pred = frames.DeviceFrame(ctx, frames.frame_format(np.uint8, hs, 0), w, h)
        assert lib.schro_frame_inverse_iwt_transform_combine_convert_hip(packed.ptr(), dev_tf.ptr(), C.byref(params), pred.ptr()) == EINVAL
        assert lib.schro_frame_inverse_iwt_transform_shift_convert_hip(packed.ptr(), dev_tf.ptr(), C.byref(params), 16) == EINVAL
        assert lib.schro_frame_inverse_iwt_transform_shift_convert_hip(packed.ptr(), dev_tf.ptr(), C.byref(params), -1) == EINVAL
        for f in (packed, pred, dev_tf):
            f.unref()
    # a non-zero shift with v210 / YUYV; shift 0 forwards to the existing call
    params, _, _, dev_tf, _ = frame_case(ctx, V216, 1, np.int16)
    for fmt in (sa.FORMAT_V210, sa.FORMAT_YUYV):
        packed, want = frames.DeviceFrame(ctx, fmt, w, h), frames.DeviceFrame(ctx, fmt, w, h)
        assert lib.schro_frame_inverse_iwt_transform_shift_convert_hip(packed.ptr(), dev_tf.ptr(), C.byref(params), 2) == EINVAL
        sa.check(lib.schro_frame_inverse_iwt_transform_shift_convert_hip(packed.ptr(), dev_tf.ptr(), C.byref(params), 0))
        sa.check(lib.schro_frame_inverse_iwt_transform_convert_hip(want.ptr(), dev_tf.ptr(), C.byref(params)))
        assert np.array_equal(np.asarray(packed.download()), np.asarray(want.download()))
        packed.unref()
        want.unref()
    dev_tf.unref()
