"""GPU: YUYV / UYVY / AYUV written by the finest wavelet level (iiwt.hip, iiwt_pack8_kernel) -- schro_hip_iiwt_pack_u8_batch.

A picture that is not a reference ends as packed bytes: the inverse wavelet, + 128 or + the prediction with the 16-bit
wrapping add and the u8 clamp, then the pack.  The LEVEL route does it without the planar picture: levels depth-1 .. 1 by
the level loop, then ONE launch that lifts the finest level of Y, U and V per tile and writes whole packed groups.  Every
case is compared bit for bit with the oracle's chain -- inverse_iwt, convert_u8 or clip (int16 (residual + prediction), 0,
255), pack_u8 --, must report its route, launch no pack ("convert" class) on the LEVEL route, and leave the bytes of dst
outside the packed rows as they were.  Full-range cases count only if the expected picture holds 0x00 and 0xff in every
component (both ends of the clamp and the wrap).  TWO_PASS pictures (4:2:0, another chroma format, s32, alignments the
kernel does not take) go through the planar picture in the queue's scratch and give the same bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import schroedinger_amd as sa
import synth
from schroedinger_amd import SubPlane, _lib, frames

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a
EINVAL = -1             # SCHRO_HIP_EINVAL (include/schro_hip.h)
YUYV, UYVY, AYUV = sa.FORMAT_YUYV, sa.FORMAT_UYVY, sa.FORMAT_AYUV
NATIVE = [(YUYV, 1, 0), (UYVY, 1, 0), (AYUV, 0, 0)]     # (format, its own chroma format)
NATIVE_IDS = ["422-yuyv", "422-uyvy", "444-ayuv"]

# The filters whose LEVEL route measured faster than the chain by more than the spread (include/schro_hip.h,
# profiles/r09_pack8_fused.txt); the others keep the two passes.  tests/test_gpu_pack8_experiments.py runs this file again
# with the experiments library and SCHRO_HIP_PACK8_LEVEL=1, where EVERY filter takes the level kernel.
LEVEL_FILTERS = {False: (3, 4, 5), True: (1, 3, 4, 5)}       # [format is AYUV]
FORCED = os.environ.get("SCHRO_HIP_PACK8_LEVEL") == "1" and "exp" in os.path.basename(os.environ.get("SCHRO_HIP_LIB", ""))


def native_route(filt, fmt):
    """The route of an s16 picture whose chroma format is the packed format's own, aligned as the level kernel asks."""
    return "level" if FORCED or filt in LEVEL_FILTERS[fmt == AYUV] else "two_pass"


def comp_dims(w, h, hs, vs):
    return [(h, w), (-(-h >> vs), -(-w >> hs)), (-(-h >> vs), -(-w >> hs))]


def coefficients(w, h, hs, vs, dtype, depth, filt, seed, full):
    dims = [(h, w), (h >> vs, w >> hs), (h >> vs, w >> hs)]
    if full:
        rng = np.random.default_rng(seed)
        return [rng.integers(-(1 << 19), 1 << 19, size=d).astype(np.int64).astype(dtype) for d in dims]
    return [O.forward_iwt((synth.image_s(a, b, dtype, seed=seed + k).astype(np.int64) * 3).astype(dtype), depth, filt)
            for k, (a, b) in enumerate(dims)]


def planar_want(co, preds, depth, filt, out_dims):
    """The planar u8 picture of the chain: convert_u8, or the prediction added with the sum wrapping to 16 bits (the last
    step of orc_rrshift6_add_s16_2d; s32 is truncated first) and clipped."""
    out = []
    for k, (oh, ow) in enumerate(out_dims):
        px = O.inverse_iwt(co[k], depth, filt)
        if preds is None:
            out.append(O.convert_u8(px, ow, oh))
        else:
            s = (px[:oh, :ow].astype(np.int64) + preds[k].astype(np.int64)).astype(np.int16)
            out.append(np.clip(s, 0, 255).astype(np.uint8))
    return out


def row_bytes(fmt, ow):
    return 4 * ow if fmt == AYUV else 4 * (ow // 2)


def run(ctx, pictures, depth, filt, dtype=np.int16, route="level", one_pack=False):
    """pictures: dicts {w, h, ow, oh, fmt, hs, vs, full, pred (bool), + optional dst_stride, pred_offset, route} -- one call.
    dst has 3 rows and 32 bytes per row more than the packed rows, all SENTINEL."""
    jobs, wants, keep, want_routes = [], [], [], {"level": 0, "two_pass": 0}
    for n, p in enumerate(pictures):
        w, h, ow, oh, fmt, hs, vs = (p[k] for k in ("w", "h", "ow", "oh", "fmt", "hs", "vs"))
        seed = 1000 * filt + 100 * depth + 10 * n + (fmt & 3)
        co = coefficients(w, h, hs, vs, dtype, depth, filt, seed, p["full"])
        out_dims = comp_dims(ow, oh, hs, vs)
        preds = d_preds = None
        if p.get("pred"):
            rng = np.random.default_rng(seed + 7)
            preds = [rng.integers(0, 256, size=d, dtype=np.uint8) for d in out_dims]
            off = p.get("pred_offset", 0)
            d_preds = []
            for a in preds:
                # the prediction's own stride (not the picture's); pred_offset: the same bytes `off` columns into a wider plane
                wide = np.zeros((a.shape[0], a.shape[1] + 8), np.uint8)
                wide[:, off:off + a.shape[1]] = a
                pl = ctx.upload(wide, stride=-(-(a.shape[1] + 8) // 8) * 8 + (3 if off else 24))
                keep.append(pl)
                d_preds.append(SubPlane(pl, 0, off, a.shape[0], a.shape[1]))
        planar = planar_want(co, preds, depth, filt, out_dims)
        if p["full"]:
            for k, a in enumerate(planar):
                assert a.min() == 0 and a.max() == 255, ("the full-range case does not reach both ends of the clamp", n, k)
        d_co = [ctx.upload(c) for c in co]
        row = row_bytes(fmt, ow)
        dst = ctx.plane(oh + 3, row + 32, np.uint8, stride=p.get("dst_stride")).fill(SENTINEL)
        jobs.append((d_co, hs, vs, d_preds, dst, ow, oh, fmt))
        wants.append((O.pack_u8(planar, hs, vs, fmt, ow, oh), row))
        keep += d_co + [dst]
        r = p.get("route", route)
        want_routes[native_route(filt, fmt) if r == "level" else r] += 1
    ctx.synchronize()
    ctx.pack8_routes(reset=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        ctx.iiwt_pack_u8_batch(jobs, depth, filt)
        ctx.synchronize()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    routes = ctx.pack8_routes(reset=True)
    case = (depth, filt, np.dtype(dtype).name)
    assert routes == want_routes, (case, routes)
    if not want_routes["two_pass"]:
        assert prof["convert"][1] == 0, (case, prof["convert"])
    if one_pack:
        assert prof["convert"][1] == 1, (case, prof["convert"])
    for n, (j, (want, row), p) in enumerate(zip(jobs, wants, pictures)):
        got = j[4].download()
        oh = p["oh"]
        if not np.array_equal(got[:oh, :row], want):
            bad = np.argwhere(got[:oh, :row] != want)
            raise AssertionError("%s picture %d %s: %d bytes differ, first at %s" % (case, n, p, len(bad), tuple(bad[0])))
        assert (got[oh:] == SENTINEL).all() and (got[:, row:] == SENTINEL).all(), ("written outside the packed rows", case, n, p)
    [q.free() for q in keep]


def batch(depth, fmt, hs, vs, pred, full):
    """Unlike pictures in one call (luma sizes multiples of 2^(depth+1)): one tile; several tiles across and down with partial
    last ones, an odd out_width and a picture smaller than its transform; a whole number of tiles' worth of columns; and
    (depths 1, 2) chroma bands whose sub-band rows are no whole 8-byte vectors."""
    sizes = [(64, 32, 64, 32), (352, 160, 333, 150), (256, 96, 256, 96), (160, 64, 148, 62)]
    if depth == 1:
        sizes.append((44, 12, 41, 11))
    if depth == 2:
        sizes.append((40, 12, 40, 9))
    return [dict(w=w, h=h, ow=ow, oh=oh, fmt=fmt, hs=hs, vs=vs, pred=pred, full=full) for (w, h, ow, oh) in sizes]


@pytest.mark.parametrize("pred", [False, True], ids=["intra", "pred"])
@pytest.mark.parametrize("fmt,hs,vs", NATIVE, ids=NATIVE_IDS)
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("filt", range(7))
def test_every_filter_depth_format_and_prediction(ctx, filt, depth, fmt, hs, vs, pred):
    run(ctx, batch(depth, fmt, hs, vs, pred, False), depth, filt)      # forward-transformed pictures
    run(ctx, batch(depth, fmt, hs, vs, pred, True), depth, filt)       # full-range coefficients


@pytest.mark.parametrize("pred", [False, True], ids=["intra", "pred"])
@pytest.mark.parametrize("fmt,hs,vs", NATIVE, ids=NATIVE_IDS)
@pytest.mark.parametrize("filt", range(7))
def test_1080_rows_inside_a_1088_row_transform(ctx, filt, fmt, hs, vs, pred):
    run(ctx, [dict(w=384, h=1088, ow=384, oh=1080, fmt=fmt, hs=hs, vs=vs, pred=pred, full=filt % 2 == 0)], 4, filt)


@pytest.mark.parametrize("filt", [0, 1])
def test_2160p(ctx, filt):
    run(ctx, [dict(w=3840, h=2160, ow=3840, oh=2160, fmt=UYVY if filt else YUYV, hs=1, vs=0, pred=True, full=False)], 3, filt)


def test_a_misaligned_prediction_takes_the_two_passes(ctx):
    # pred three bytes into its plane and a stride of 3 mod 8: the level kernel reads prediction rows in 8-byte words
    for (fmt, hs, vs) in NATIVE:
        run(ctx, [dict(w=352, h=160, ow=333, oh=150, fmt=fmt, hs=hs, vs=vs, pred=True, full=True, pred_offset=3)], 3, 0,
            route="two_pass")


@pytest.mark.parametrize("fmt", [YUYV, UYVY, AYUV], ids=["yuyv", "uyvy", "ayuv"])
def test_two_pass_pictures(ctx, fmt):
    own = (0, 0) if fmt == AYUV else (1, 0)
    other = (1, 0) if fmt == AYUV else (0, 0)
    base = dict(w=352, h=160, ow=333, oh=150, fmt=fmt, full=False)
    for pred in (False, True):
        # 4:2:0 (chroma rows repeated), a source whose chroma format is not the destination's
        run(ctx, [dict(base, hs=1, vs=1, pred=pred), dict(base, hs=other[0], vs=other[1], pred=pred, full=True)], 3, 1, route="two_pass")
        # s32 sources
        run(ctx, [dict(base, hs=own[0], vs=own[1], pred=pred, full=True)], 2, 0, dtype=np.int32, route="two_pass")
        # a dst stride that is no multiple of 16 (8 or 4 mod 16)
        run(ctx, [dict(base, hs=own[0], vs=own[1], pred=pred, dst_stride=row_bytes(fmt, 333) + 32)], 3, 6, route="two_pass")


@pytest.mark.parametrize("depth", [1, 3])
def test_level_and_two_pass_pictures_in_one_call(ctx, depth):
    # the level pictures' LL planes and the two-pass pictures' planar pictures share the queue's block, each at its own
    # offset; the two-pass pictures (s16, Haar, aligned: the combine form writes them directly) make ONE pack launch
    pics = [dict(w=352, h=160, ow=333, oh=150, fmt=YUYV, hs=1, vs=0, pred=True, full=False, route="level"),
            dict(w=352, h=160, ow=352, oh=160, fmt=UYVY, hs=1, vs=0, pred=True, full=True, dst_stride=4 * 176 + 40, route="two_pass"),
            dict(w=256, h=96, ow=256, oh=96, fmt=AYUV, hs=0, vs=0, pred=False, full=True, route="level"),
            dict(w=256, h=128, ow=256, oh=128, fmt=YUYV, hs=0, vs=0, pred=False, full=False, route="two_pass"),
            dict(w=384, h=1088, ow=384, oh=1080, fmt=UYVY, hs=1, vs=0, pred=False, full=False, route="level")]
    run(ctx, pics, depth, 3, one_pack=True)


def test_refusals_launch_and_count_nothing(ctx):
    co = [ctx.upload(np.zeros(d, np.int16)) for d in [(32, 64), (32, 32), (32, 32)]]
    pr = [ctx.upload(np.zeros(d, np.uint8)) for d in [(32, 64), (32, 32), (32, 32)]]
    dst = ctx.plane(32, 128, np.uint8)
    ctx.synchronize()
    ctx.pack8_routes(reset=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        good = (co, 1, 0, pr, dst, 64, 32, YUYV)
        bad = [
            (good[:7] + (sa.FORMAT_V210,), 3, 0),                            # a format other than the three
            (good[:5] + (66, 32, YUYV), 3, 0),                               # out_width outside the transform
            (good[:5] + (64, 33, YUYV), 3, 0),                               # out_height outside the transform
            (good, 6, 0),                                                    # 64 x 32 is not a multiple of 2^6
        ]
        bad = [(job, depth, 3) for (job, depth, _) in bad]                   # (Haar: the good picture takes LEVEL)
        for job, depth, filt in bad:
            with pytest.raises(sa.SchroHipError):
                ctx.iiwt_pack_u8_batch([job], depth, filt)
        # a prediction for some components only
        arr = (_lib.IwtPack8Picture * 1)()
        a = arr[0]
        for k in range(3):
            a.src[k], a.src_stride[k] = co[k].ptr, co[k].stride
            a.pred[k], a.pred_stride[k] = pr[k].ptr, pr[k].stride
        a.width, a.height, a.h_shift, a.v_shift = 64, 32, 1, 0
        a.dst, a.dst_stride, a.out_width, a.out_height, a.format = dst.ptr, dst.stride, 64, 32, YUYV
        assert ctx.lib.schro_hip_iiwt_pack_u8_batch(ctx.h, arr, 1, 3, 3, 2) == 0
        ctx.synchronize()
        good_prof = ctx.profile_read()          # (the launches of the one good call: the refused calls add none)
        a.pred[1] = None
        assert ctx.lib.schro_hip_iiwt_pack_u8_batch(ctx.h, arr, 1, 3, 3, 2) == EINVAL
        a.pred[1] = pr[1].ptr
        a.pred_stride[2] = 31                                                # shorter than the component's out width
        assert ctx.lib.schro_hip_iiwt_pack_u8_batch(ctx.h, arr, 1, 3, 3, 2) == EINVAL
        a.pred_stride[2] = pr[2].stride
        a.src_stride[0] = 126                                                # shorter than a row
        assert ctx.lib.schro_hip_iiwt_pack_u8_batch(ctx.h, arr, 1, 3, 3, 2) == EINVAL
        a.src_stride[0] = co[0].stride
        assert ctx.lib.schro_hip_iiwt_pack_u8_batch(ctx.h, arr, 1, 3, 3, 3) == EINVAL      # bytes_per_sample
        # a good picture behind a bad one in the same call: nothing launched, nothing counted
        two = (_lib.IwtPack8Picture * 2)()
        C.memmove(C.addressof(two[0]), C.addressof(arr[0]), C.sizeof(_lib.IwtPack8Picture))
        C.memmove(C.addressof(two[1]), C.addressof(arr[0]), C.sizeof(_lib.IwtPack8Picture))
        two[1].format = 0x103
        assert ctx.lib.schro_hip_iiwt_pack_u8_batch(ctx.h, two, 2, 3, 3, 2) == EINVAL
        ctx.synchronize()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    assert ctx.pack8_routes(reset=True) == {"level": 1, "two_pass": 0}       # (the one good call above)
    assert {k: v[1] for k, v in prof.items()} == {k: v[1] for k, v in good_prof.items()} and prof["convert"][1] == 0, (prof, good_prof)
    [p.free() for p in co + pr + [dst]]


def up(v, depth):
    return -(-v // (1 << depth)) * (1 << depth)


def test_end_to_end_against_the_motion_render(ctx):
    """The prediction rendered by schro_hip_obmc_batch (prediction_only = 1), the picture packed by the level route: the
    oracle's motion render over the inverse transform's output, then pack_u8."""
    w, h, depth, filt, prec, hs, vs = 320, 240, 3, 4, 2, 1, 0
    dims = comp_dims(w, h, hs, vs)
    iw = [(up(ph, depth), up(pw, depth)) for (ph, pw) in dims]
    resid = [(synth.image_s(ih, iwd, np.int16, seed=3 + k).astype(np.int64) * 3).astype(np.int16) for k, (ih, iwd) in enumerate(iw)]
    coeffs = [O.forward_iwt(r, depth, filt) for r in resid]
    res_want = [O.inverse_iwt(c, depth, filt) for c in coeffs]
    d_co = [ctx.upload(c) for c in coeffs]
    P = synth.motion_params(w, h, 12, 8, prec, (1, 1, 1), (hs, vs))
    mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 20 << prec, 9)
    d_mv = ctx.upload_bytes(mv)
    refs_np = [[synth.picture_u8(ph, pw, seed=11 + 10 * r + k) for k, (ph, pw) in enumerate(dims)] for r in range(2)]
    hp, keep = [], list(d_co) + [d_mv]
    for r in range(2):
        g0 = ctx.hp_plane(*dims[0])
        ctx.upsample_batch([(ctx.upload(refs_np[r][0]), g0)])
        gp = ctx.hp_plane(*dims[1], pair=True)
        ctx.upsample_batch([((ctx.upload(refs_np[r][1]), ctx.upload(refs_np[r][2])), gp)])
        hp.append([g0, gp, gp])
        keep += [g0, gp]
    preds = [ctx.plane(ph, pw, np.uint8).fill(0xa1) for (ph, pw) in dims]
    ctx.obmc_batch([sa.obmc_plane(d_mv, P, k, hp[0][k], hp[1][k], None, preds[k], prediction_only=True) for k in range(3)])
    want_planar = [O.motion_render(mv, O.MotionParams(**P), k, O.UpComp(refs_np[0][k], upsample=True), O.UpComp(refs_np[1][k], upsample=True),
                                   res_want[k], pw, ph) for k, (ph, pw) in enumerate(dims)]
    for fmt in (YUYV, UYVY):
        dst = ctx.plane(h, row_bytes(fmt, w), np.uint8).fill(SENTINEL)
        ctx.pack8_routes(reset=True)
        ctx.iiwt_pack_u8_batch([(d_co, hs, vs, preds, dst, w, h, fmt)], depth, filt)
        ctx.synchronize()
        assert ctx.pack8_routes(reset=True) == {"level": 1, "two_pass": 0}
        assert np.array_equal(dst.download(), O.pack_u8(want_planar, hs, vs, fmt, w, h)), fmt
        dst.free()
    [p.free() for p in keep + preds]


@pytest.mark.parametrize("fmt,hs,vs,dtype", [(UYVY, 1, 0, np.int16), (AYUV, 0, 0, np.int16), (YUYV, 1, 1, np.int16), (UYVY, 1, 0, np.int32)],
                         ids=["uyvy-422", "ayuv-444", "yuyv-420", "uyvy-422-s32"])
def test_frame_layer_calls(ctx, fmt, hs, vs, dtype):
    """schro_frame_inverse_iwt_transform_convert_hip with a packed 8-bit frame and _combine_convert_hip with the prediction of
    schro_motion_render_hip (add = FALSE) equal schro_frame_inverse_iwt_transform_combine_hip + schro_hipframe_convert."""
    w, h, depth, filt, prec = 320, 240, 3, 1, 2
    lib = ctx.lib
    pd = comp_dims(w, h, hs, vs)
    iw = [(up(ph, depth), up(pw, depth)) for (ph, pw) in pd]
    P = synth.motion_params(w, h, 12, 8, prec, (1, 1, 1), (hs, vs))
    params = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=iw[0][1], iwt_luma_height=iw[0][0],
                                iwt_chroma_width=iw[1][1], iwt_chroma_height=iw[1][0], num_refs=2,
                                **{k: P[k] for k in ("xblen_luma", "yblen_luma", "xbsep_luma", "ybsep_luma", "mv_precision",
                                                     "picture_weight_bits", "picture_weight_1", "picture_weight_2", "x_num_blocks", "y_num_blocks")})
    mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 24 << prec, seed=4)
    coeffs = [O.forward_iwt(synth.image_s(ih, iwd, dtype, seed=20 + k), depth, filt) for k, (ih, iwd) in enumerate(iw)]
    fmt_t, fmt8 = frames.frame_format(dtype, hs, vs), frames.frame_format(np.uint8, hs, vs)
    dev_tf = frames.DeviceFrame(ctx, fmt_t, iw[0][1], iw[0][0]).upload(frames.HostFrame(coeffs, hs, vs))
    refs = []
    for r in range(2):
        planes = [synth.picture_u8(ph, pw, seed=40 + 10 * r + k) for k, (ph, pw) in enumerate(pd)]
        d = frames.DeviceFrame(ctx, fmt8, w, h).upload(frames.HostFrame(planes, hs, vs))
        u = frames.DeviceFrame(ctx, fmt8, w, h, upsampled=True)
        sa.check(lib.schro_upsampled_hipframe_upsample(u.ptr(), d.ptr()))
        refs += [u]
        d.unref()
    mc_tmp, planar = frames.DeviceFrame(ctx, fmt8, w, h), frames.DeviceFrame(ctx, fmt8, w, h)
    motion = _lib.Motion(refs[0].ptr(), refs[1].ptr(), mv.ctypes.data, C.pointer(params))
    sa.check(lib.schro_motion_render_hip(C.byref(motion), mc_tmp.ptr(), None, 0, None))
    for prediction in (None, mc_tmp):
        want, got = frames.DeviceFrame(ctx, fmt, w, h), frames.DeviceFrame(ctx, fmt, w, h)
        sa.check(lib.schro_frame_inverse_iwt_transform_combine_hip(planar.ptr(), dev_tf.ptr(), C.byref(params),
                                                                   prediction.ptr() if prediction else None))
        sa.check(lib.schro_hipframe_convert(want.ptr(), planar.ptr()))
        ctx.pack8_routes(reset=True)
        if prediction is None:
            sa.check(lib.schro_frame_inverse_iwt_transform_convert_hip(got.ptr(), dev_tf.ptr(), C.byref(params)))
        else:
            sa.check(lib.schro_frame_inverse_iwt_transform_combine_convert_hip(got.ptr(), dev_tf.ptr(), C.byref(params), prediction.ptr()))
        level = dtype == np.int16 and vs == 0 and native_route(filt, fmt) == "level"
        assert ctx.pack8_routes(reset=True) == {"level": int(level), "two_pass": int(not level)}
        assert np.array_equal(got.download(), want.download()), "with a prediction" if prediction else "without"
        want.unref()
        got.unref()
    for f in (mc_tmp, planar, dev_tf) + tuple(refs):
        f.unref()
