"""GPU: the v210 copy-out written by the finest wavelet level for every filter and depth (iiwt.hip, iiwt_v210_kernel).

schro_hip_iiwt_pack_v210_batch hands every 4:2:2 picture that the three-level s32 Haar kernel does not take to the level
route: levels depth-1 .. 1 by the level loop into compact LL planes, then ONE launch whose tiles lift the finest level of
Y, U and V and pack their v210 groups -- no pixel frame, no pack launch.  Each case is compared bit for bit with the
oracle's chain (inverse wavelet, crop, pack_v210_s16), with full-range coefficients (the s32 -> s16 truncation, the
16-bit wrap points and the 10-bit clamp) and transformed pictures; each call must report the level route, launch no
pack ("convert" class), and leave the bytes of dst outside the picture's v210 rows as they were."""
import numpy as np
import pytest

import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a


def coefficients(h, w, dtype, depth, filt, seed, full):
    dims = [(h, w), (h, w >> 1), (h, w >> 1)]
    if full:
        rng = np.random.default_rng(seed)
        return [rng.integers(-(1 << 19), 1 << 19, size=d).astype(np.int64).astype(dtype) for d in dims]
    return [O.forward_iwt((synth.image_s(a, b, dtype, seed=seed + k).astype(np.int64) * 3).astype(dtype), depth, filt)
            for k, (a, b) in enumerate(dims)]


def want_v210(co, depth, filt, ow, oh):
    px = [O.inverse_iwt(c, depth, filt) for c in co]
    return O.pack_v210([p[:oh, :(ow if k == 0 else -(-ow // 2))] for k, p in enumerate(px)], 1, 0, ow, oh)


def run(ctx, pictures, depth, filt, dtype, route="level"):
    """pictures: (w, h, out_w, out_h, full-range[, dst stride]) per picture, one call.  dst has 3 rows and 32 bytes per row
    more than the picture's v210 rows, all filled with SENTINEL.  route: the route of every picture, or {route: pictures}."""
    jobs, wants, keep = [], [], []
    for n, (w, h, ow, oh, full, *stride) in enumerate(pictures):
        co = coefficients(h, w, dtype, depth, filt, 100 * filt + 10 * depth + n, full)
        d_co = [ctx.upload(c) for c in co]
        row = 16 * (-(-ow // 6))
        dst = ctx.plane(oh + 3, row + 32, np.uint8, stride=stride[0] if stride else None).fill(SENTINEL)
        jobs.append((d_co, 1, 0, dst, ow, oh))
        wants.append((want_v210(co, depth, filt, ow, oh), row))
        keep += d_co + [dst]
    ctx.synchronize()
    ctx.v210_routes(reset=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        ctx.iiwt_pack_v210_batch(jobs, depth, filt)
        ctx.synchronize()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    routes = ctx.v210_routes(reset=True)
    case = (depth, filt, np.dtype(dtype).name)
    want_routes = {"haar3": 0, "level": 0, "two_pass": 0}
    want_routes.update({route: len(pictures)} if isinstance(route, str) else route)
    assert routes == want_routes, (case, routes)
    # (the pack of the two-pass pictures, if any, is one launch)
    assert prof["convert"][1] == (1 if want_routes["two_pass"] else 0), (case, prof["convert"])
    for (j, (want, row), (w, h, ow, oh, full, *_)) in zip(jobs, wants, pictures):
        got = j[3].download()
        assert np.array_equal(got[:oh, :row], want), (case, w, h, ow, oh, full)
        assert (got[oh:] == SENTINEL).all() and (got[:, row:] == SENTINEL).all(), ("written outside the picture", case, w, h, ow, oh)
    [p.free() for p in keep]


def batch(depth):
    """Pictures of different sizes in one call (luma widths multiples of 2^(depth+1): 4:2:2 chroma is a whole transform too):
    48 x 8 (64 x 16 at depth 4), a width that is no multiple of 6 inside its transform, several tiles across and down
    with partial last ones, and (depths 1, 2) chroma bands whose sub-band rows are no whole 8-byte vectors -- the loads
    without them."""
    pics = [(48, 8, 48, 8, True)] if depth <= 3 else [(64, 16, 64, 16, True)]
    pics += [(160, 32, 148, 30, False), (224, 48, 221, 48, True), (96, 144, 96, 137, False)]
    if depth == 1:
        pics.append((44, 12, 41, 11, True))
    if depth == 2:
        pics.append((40, 12, 40, 9, True))
    return pics


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("filt", range(7))
def test_every_filter_depth_and_sample_type(ctx, filt, depth, dtype):
    run(ctx, batch(depth), depth, filt, dtype)


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("filt", range(7))
def test_1080_rows_inside_a_1088_row_transform(ctx, filt, dtype):
    run(ctx, [(1920, 1088, 1920, 1080, filt % 2 == 0)], 4, filt, dtype)


@pytest.mark.parametrize("filt", [0, 1])
def test_8k(ctx, filt):
    run(ctx, [(7680, 4320, 7680, 4320, False)], 3, filt, np.int32)


def test_config5_haar_keeps_its_kernel(ctx):
    # the three-level s32 Haar of a picture whose size is a multiple of 192 x 8 stays on iiwt_haar3_v210_kernel
    for filt in (3, 4):
        run(ctx, [(192, 16, 192, 16, True), (960, 64, 960, 64, False)], 3, filt, np.int32, route="haar3")


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("filt", [0, 5])
def test_level_and_two_pass_pictures_in_one_call(ctx, filt, depth, dtype):
    # a dst stride of 8 mod 16 sends a picture to the two passes; the level pictures' LL planes and the two-pass picture's
    # pixel frame then share the queue's block, each at its own offset
    row = 16 * (-(-148 // 6))
    pics = [(160, 32, 148, 30, False, row + 40), (224, 48, 221, 48, True), (96, 144, 96, 137, True, 16 * 16 + 40),
            (1920, 1088, 1920, 1080, False)]
    run(ctx, pics, depth, filt, dtype, route={"level": 2, "two_pass": 2})
