"""GPU: level 1 of the inverse wavelet synthesised inside the level-0 register tile (iiwt_reg.hip, MODE bit 8).

A batch whose level 0 takes the large register tile runs level 1 of every plane that allows it inside the level-0
launch: the tile makes its LL band from the level-1 sub-bands in registers.  Every case here is compared bit for bit
with the oracle -- the plain s16 output (MODE 0) and the combine form (MODE 4) with a prediction and without one
(intra: + 128), every filter of the register form (those it is not built for keep a launch per level), depths 2 .. 4, planes of
2160p and 1080p luma and chroma and a size whose last tile row and column are partial, and the transform in two calls.
The batches carry two 2160p luma planes so that level 0 takes the large tile, as the headline's batches do."""
import numpy as np
import pytest

import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

FILTERS = [0, 1, 2, 3, 4, 6]
INLINE = (0, 6)                 # the filters the form is built for: DD(9,7), Daub(9,7)


def sizes(depth):
    # 2160p luma twice (the batch's level 0 is then >= 2048 tiles: the large tile), 1080p luma, 2160p chroma, and
    # 1056 x 600: 528 sub-band columns (tiles of 240: the last one partial) and 300 row pairs (the last tile row moved up)
    h1080 = 1088 if depth == 4 else 1080
    return [(2160, 3840), (2160, 3840), (h1080, 1920), (h1080, 1920), (608 if depth == 4 else 600, 1056)]


_cache = {}


def coefficients(filt, depth):
    key = (filt, depth)
    if key not in _cache:
        co, want = [], []
        for k, (h, w) in enumerate(sizes(depth)):
            img = synth.image_s(h, w, np.int16, seed=11 * filt + 3 * depth + k)
            c = O.forward_iwt(img, depth, filt)
            co.append(c)
            want.append(O.inverse_iwt(c, depth, filt))
        if len(_cache) >= 6:
            _cache.pop(next(iter(_cache)))
        _cache[key] = (co, want)
    return _cache[key]


def level_launches(ctx, run):
    ctx.profile_reset()
    ctx.profile_enable(True)
    run()
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return prof["iiwt_finest"][1], prof["iiwt_coarse"][1]


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("filt", FILTERS)
def test_plain_output(ctx, filt, depth):
    co, want = coefficients(filt, depth)
    d_co = [ctx.upload(c) for c in co]
    outs = [ctx.plane(c.shape[0], c.shape[1], np.int16).fill(0x5e) for c in co]
    fin, coarse = level_launches(ctx, lambda: ctx.iiwt_batch(list(zip(d_co, outs)), depth, filt))
    for k in range(len(co)):
        got = outs[k].download()
        if not np.array_equal(got, want[k]):
            bad = np.argwhere(got != want[k])
            raise AssertionError("plane %d %s: %d mismatches, first at %s" % (k, co[k].shape, len(bad), tuple(bad[0])))
    if depth == 2:
        # level 1 inside level 0: no launch of a coarser level at all
        assert (fin, coarse) == ((1, 0) if filt in INLINE else (1, 1)), (fin, coarse)
    [p.free() for p in d_co + outs]


@pytest.mark.parametrize("intra", [False, True])
@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("filt", FILTERS)
def test_combine_form(ctx, filt, depth, intra):
    co, res = coefficients(filt, depth)
    d_co = [ctx.upload(c) for c in co]
    # the picture inside the transform's size: a few columns and rows short of it where the plane allows
    dims = [(h - (2 if k == 4 else 0), w - (8 if k == 4 else 0)) for k, (h, w) in enumerate(c.shape for c in co)]
    outs = [ctx.plane(ph, pw, np.uint8).fill(0x5e) for (ph, pw) in dims]
    preds_np = [synth.picture_u8(ph, pw, seed=5 + k) for k, (ph, pw) in enumerate(dims)]
    preds = [None] * len(co) if intra else [ctx.upload(p) for p in preds_np]
    fin, coarse = level_launches(ctx, lambda: ctx.iiwt_batch([(d_co[k], outs[k], preds[k]) for k in range(len(co))], depth, filt))
    for k, (ph, pw) in enumerate(dims):
        if intra:
            want = O.convert_u8(res[k], pw, ph)
        else:
            # sat_u8 (residual + prediction) with the reference's 16-bit wrapping add
            want = np.clip((res[k][:ph, :pw] + preds_np[k].astype(np.int16)).astype(np.int16), 0, 255).astype(np.uint8)
        got = outs[k].download()
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError("plane %d %s: %d mismatches, first at %s" % (k, (ph, pw), len(bad), tuple(bad[0])))
    if depth == 2:
        assert (fin, coarse) == ((1, 0) if filt in INLINE else (1, 1)), (fin, coarse)
    [p.free() for p in d_co + outs + [p for p in preds if p is not None]]


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("filt", INLINE)
def test_transform_in_two_calls(ctx, filt, depth):
    """levels >= 2 on the level-2 view into an LL plane of the caller's, then levels 1 and 0 with that plane as the LL
    band of level 1 -- which the level-0 tiles now read themselves"""
    co, want = coefficients(filt, depth)
    d_co = [ctx.upload(c) for c in co]
    outs = [ctx.plane(c.shape[0], c.shape[1], np.int16) for c in co]
    lls = [ctx.plane(c.shape[0] // 4, c.shape[1] // 4, np.int16) for c in co]
    if depth > 2:
        ctx.iiwt_batch([(d.level_view(2), ll) for d, ll in zip(d_co, lls)], depth - 2, filt)
    else:
        for c, ll in zip(co, lls):      # (the LL band of the level-1 view: every fourth row, its first w / 4 columns)
            ll.upload(np.ascontiguousarray(c[::4, :c.shape[1] // 4]))
    fin, coarse = level_launches(ctx, lambda: ctx.iiwt_batch(list(zip(d_co, outs)), 2, filt, ll=lls))
    assert (fin, coarse) == (1, 0), (fin, coarse)
    for k in range(len(co)):
        assert np.array_equal(outs[k].download(), want[k]), (k, co[k].shape)
    [p.free() for p in d_co + outs + lls]
