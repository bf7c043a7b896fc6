"""GPU: what the three fused wavelet-to-packed-picture calls share on the host (iiwt_pack.cpp) -- schro_hip_iiwt_pack_v210_batch,
schro_hip_iiwt_pack_u8_batch and schro_hip_iiwt_pack_wide_batch.

The queue's grow-only block: the three calls lay their compact LL planes (LEVEL) and their pixel planes (TWO_PASS) out in
ONE block per queue, reused in order on the queue.  A sequence of unlike calls with no host synchronise between them --
the block grows twice and is then reused by a call that needs less -- must give the oracle's bytes for every picture, on
both queues.

The refusals: the three calls refuse through the same checks, which take the call's name; each text is pinned to a
literal, and a refused call launches and counts nothing wherever its bad picture stands."""
import numpy as np
import pytest

import oracle_lib as O
import schroedinger_amd as sa
import test_gpu_pack8_fused as P8
import test_gpu_v210_every_filter as V2
import test_gpu_wide_fused as WD
from schroedinger_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a
EINVAL = -1             # SCHRO_HIP_EINVAL (include/schro_hip.h)


def v210_case(ctx):
    """A v210 LEVEL picture, s16, 96 x 16, depth 2 (LeGall): three LL planes of 1 KiB in the block."""
    w, h, depth, filt = 96, 16, 2, 1
    co = V2.coefficients(h, w, np.int16, depth, filt, 11, False)
    want = V2.want_v210(co, depth, filt, w, h)
    dst = ctx.plane(h, want.shape[1], np.uint8)
    job = ([ctx.upload(c) for c in co], 1, 0, dst, w, h)
    return (lambda: ctx.iiwt_pack_v210_batch([job], depth, filt)), dst, want, job[0] + [dst]


def ayuv_case(ctx):
    """An AYUV LEVEL picture with a prediction, s16, 192 x 32, depth 3, filter 3 (Haar): three LL planes of 4 KiB."""
    w, h, depth, filt = 192, 32, 3, 3
    co = P8.coefficients(w, h, 0, 0, np.int16, depth, filt, 23, False)
    dims = P8.comp_dims(w, h, 0, 0)
    rng = np.random.default_rng(29)
    preds = [rng.integers(0, 256, size=d, dtype=np.uint8) for d in dims]
    want = O.pack_u8(P8.planar_want(co, preds, depth, filt, dims), 0, 0, sa.FORMAT_AYUV, w, h)
    dst = ctx.plane(h, want.shape[1], np.uint8)
    d_co, d_pr = [ctx.upload(c) for c in co], [ctx.upload(a) for a in preds]
    job = (d_co, 0, 0, d_pr, dst, w, h, sa.FORMAT_AYUV)
    return (lambda: ctx.iiwt_pack_u8_batch([job], depth, filt)), dst, want, d_co + d_pr + [dst]


def ay64_case(ctx):
    """An AY64 TWO_PASS picture (a dst stride of 8 mod 16), s32, 384 x 64, depth 3: three pixel planes of 96 KiB."""
    w, h, depth, filt, shift = 384, 64, 3, 0, 2
    co = WD.coefficients(w, h, 0, np.int32, depth, filt, 37, True)
    want = WD.oracle_bytes(co, depth, filt, 0, w, h, sa.FORMAT_AY64, shift)
    dst = ctx.plane(h, want.shape[1], np.uint8, stride=want.shape[1] + 8)
    job = ([ctx.upload(c) for c in co], 0, 0, dst, w, h, sa.FORMAT_AY64, shift)
    return (lambda: ctx.iiwt_pack_wide_batch([job], depth, filt)), dst, want, job[0] + [dst]


def test_the_block_is_shared_by_the_three_calls():
    ctx = sa.Context(0)         # (a context of its own: both queues' blocks begin empty)
    try:
        cases = [v210_case(ctx), ayuv_case(ctx), ay64_case(ctx)]
        for q in (0, 1):
            for _, dst, _, _ in cases:
                dst.fill(SENTINEL)
            first_again = ctx.plane(cases[0][1].height, cases[0][1].width, np.uint8).fill(SENTINEL)
            ctx.synchronize()
            for read in (ctx.v210_routes, ctx.pack8_routes, ctx.wide_routes):
                read(reset=True)
            ctx.select_queue(q)
            for call, _, _, _ in cases:
                call()          # (the block grows at the second and at the third)
            # the first picture again, into another dst: the block is larger than it needs
            planes = cases[0][3][:3]
            ctx.iiwt_pack_v210_batch([(planes, 1, 0, first_again, 96, 16)], 2, 1)
            ctx.synchronize()
            ctx.select_queue(0)
            assert ctx.v210_routes(reset=True) == {"haar3": 0, "level": 2, "two_pass": 0}, q
            assert ctx.pack8_routes(reset=True) == {"level": 1, "two_pass": 0}, q
            assert ctx.wide_routes(reset=True) == {"level": 0, "two_pass": 1}, q
            for n, (_, dst, want, _) in enumerate(cases):
                assert np.array_equal(dst.download(), want), (q, n)
            assert np.array_equal(first_again.download(), cases[0][2]), (q, "the first picture again")
            first_again.free()
    finally:
        ctx.close()


def fill(a, planes, hs, dst, **more):
    for k in range(3):
        a.src[k], a.src_stride[k] = planes[k].ptr, planes[k].stride
    a.width, a.height, a.h_shift, a.v_shift = 64, 32, hs, 0
    a.dst, a.dst_stride, a.out_width, a.out_height = dst.ptr, dst.stride, 64, 32
    for k, v in more.items():
        setattr(a, k, v)


# (call, its picture struct, its route reader, what else a good 64 x 32 4:2:2 s16 picture sets, the call's own refusal: the
# field to spoil, the value, the text behind "<call>: picture 1")
CALLS = {
    "v210": ("iiwt_pack_v210_batch", "IwtPackPicture", "v210_routes", {}, ("h_shift", 0, ": v210 from s16 / s32 frames needs a 4:2:2 frame")),
    "u8": ("iiwt_pack_u8_batch", "IwtPack8Picture", "pack8_routes", {"format": sa.FORMAT_YUYV},
           ("pred", 1, ": a prediction for some components and not for others")),
    "wide": ("iiwt_pack_wide_batch", "IwtPackWidePicture", "wide_routes", {"format": sa.FORMAT_V216}, ("shift", 16, ": shift 16")),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_refusal_texts(ctx, name):
    """Bad geometry, a component that is no multiple of 2^depth, a short src_stride and the call's own refusal, each in the
    SECOND picture of a call behind a good one: the text of schro_hip_last_error, nothing launched, nothing counted."""
    who, struct, routes, more, (own_field, own_value, own_text) = CALLS[name]
    co = [ctx.upload(np.zeros(d, np.int16)) for d in [(32, 64), (32, 32), (32, 32)]]
    pr = [ctx.upload(np.zeros(d, np.uint8)) for d in [(32, 64), (32, 32), (32, 32)]]
    dst = [ctx.plane(32, 512, np.uint8).fill(SENTINEL) for _ in range(2)]
    arr = (getattr(_lib, struct) * 2)()
    call = lambda depth=3: getattr(ctx.lib, "schro_hip_" + who)(ctx.h, arr, 2, depth, 1, 2)

    def good():
        for a, d in zip(arr, dst):
            fill(a, co, 1, d, **more)
            for k in range(3 if name == "u8" else 0):
                a.pred[k], a.pred_stride[k] = pr[k].ptr, pr[k].stride

    ctx.synchronize()
    getattr(ctx, routes)(reset=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        b = arr[1]
        good()
        b.out_width = 66
        assert call() == EINVAL
        assert ctx.lib.schro_hip_last_error().decode() == who + ": picture 1: bad geometry"
        good()
        assert call(depth=6) == EINVAL          # (the FIRST picture is as bad: it is the one named)
        assert ctx.lib.schro_hip_last_error().decode() == who + ": picture 0 component 0: size 64x32 is not a multiple of 2^depth"
        good()
        b.src_stride[1] = 62
        assert call() == EINVAL
        assert ctx.lib.schro_hip_last_error().decode() == who + ": picture 1 component 1: stride 62 does not hold 32 samples"
        good()
        if own_field == "pred":
            b.pred[own_value] = None
        else:
            setattr(b, own_field, own_value)
        assert call() == EINVAL
        assert ctx.lib.schro_hip_last_error().decode() == who + ": picture 1" + own_text
        ctx.synchronize()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    assert all(v[1] == 0 for v in prof.values()), prof
    assert not any(getattr(ctx, routes)(reset=True).values())
    assert all((d.download() == SENTINEL).all() for d in dst)
    [p.free() for p in co + pr + dst]
