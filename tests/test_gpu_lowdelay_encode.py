"""GPU parity: the low-delay slice encoder (schro_hip_lowdelay_encode_batch, schro_hip_encode_lowdelay_transform_data)
against tests/lowdelay_enc_ref.py: the bytes, the base indices and the over-run count, exactly.  The checker restates
schro_encoder_encode_lowdelay_transform_data and is held by tests/test_lowdelay_enc_ref.py.  Every call runs on guarded
memory (tests/guard_lib.py): nothing outside the slice buffer, the index array and the count is written, and the
coefficient planes -- with padded strides -- are left as they were."""
import ctypes as C

import numpy as np
import pytest

import guard_lib as G
import lowdelay_enc_cases as K
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu


def run(ctx, P, pictures, pads=(0, 6, 64), skew=0):
    """One call over `pictures` (lists of three planes); returns per picture (bytes, indices, count) after the footprint
    check.  The planes get strides padded by pads[k] bytes; the slice buffers start `skew` bytes off a 256-byte line."""
    lay = G.Layout()
    nslices = P["n_horiz_slices"] * P["n_vert_slices"]
    nbytes = P["slice_bytes_num"] * nslices // P["slice_bytes_denom"]
    specs = []
    for planes in pictures:
        comp = [lay.plane(p.shape[0], p.shape[1], np.int16, stride=p.shape[1] * 2 + pads[k], footprint=None, name="comp%d" % k)
                for k, p in enumerate(planes)]
        specs.append((comp, lay.span(nbytes, skew=skew, footprint=("bytes", nbytes), name="slices"),
                      lay.span(nslices, skew=1, footprint=("bytes", nslices), name="index"),
                      lay.span(4, footprint=("bytes", 4), name="count")))
    blk = G.GuardedBlock(ctx, lay, seed=nbytes)
    try:
        for planes, (comp, _, _, _) in zip(pictures, specs):
            for k in range(3):
                blk[comp[k]].upload(planes[k])
        ctx.lowdelay_encode_batch([([blk[c] for c in comp], blk[sl], blk[ix], blk[cn]) for comp, sl, ix, cn in specs], P)
        ctx.synchronize()
        raw = blk.raw()
        blk.check()             # strays; the inputs declare an empty footprint: they are unchanged
        return [(sl.payload(raw)[0], ix.payload(raw)[0], int(cn.payload(raw).view(np.uint32)[0, 0])) for _, sl, ix, cn in specs]
    finally:
        blk.free()


def assert_same(got, res):
    data, index, count = got
    assert index.tolist() == res["index"].tolist()
    assert count == res["count"]
    bad = np.flatnonzero(data != res["bytes"])
    assert bad.size == 0, "%d bytes differ, first at %d" % (bad.size, bad[0])


@pytest.mark.parametrize("name", list(K.CASES) + ["span"])
def test_bytes_indices_and_count(ctx, name):
    """Depths 1 .. 4 x three chroma formats with fractional slice sizes; 1 x 1 LL blocks on a long diagonal chain; unequal
    rectangles; one slice for a whole picture (the looping paths); base - matrix below 0; full-range values (the LL wrap);
    all zero; over-run slices (cut and counted); indices spanning 0 .. 64; the serial launch off LDS with several threads
    (spill_2x2, spill_3x5_420: lowdelay_enc_cases.leaves_lds)."""
    P, planes, res = K.expected(name)
    assert_same(run(ctx, P, [planes])[0], res)


@pytest.mark.parametrize("index", [0, 32])
def test_exact_fits(ctx, index):
    """the estimate meets the budget to the bit: at index 0 the slice stays (<=), in the loop it moves up (>=)"""
    P, planes, res = K.exact_fit(index)
    assert_same(run(ctx, P, [planes], skew=3)[0], res)


def test_batch_of_three_unlike_pictures(ctx):
    P = K.CASES["64x32_d3_422"][0]
    pics = [K.coefficients(P, kind, seed) for kind, seed in (("small", 41), ("full", 42), ("zero", 0))]
    import lowdelay_enc_ref as R
    got = run(ctx, P, pics, pads=(2, 30, 0), skew=1)
    for g, planes in zip(got, pics):
        assert_same(g, R.encode(planes, P))


def test_batch_of_three_unlike_pictures_off_lds(ctx):
    """the spill_2x2 geometry, whose serial launch keeps its samples in the queue's scratch: three pictures' regions of it
    live at once, each with two threads on the middle diagonal"""
    import lowdelay_enc_ref as R
    name, kinds = K.SPILL_BATCH
    P = K.CASES[name][0]
    assert K.leaves_lds(P)
    pics = [K.coefficients(P, kind, seed) for kind, seed in kinds]
    got = run(ctx, P, pics, pads=(2, 30, 0), skew=1)
    for g, planes in zip(got, pics):
        assert_same(g, R.encode(planes, P))


def test_large_picture(ctx):
    """960 x 540 4:2:2 at depth 3 in 30 x 68 slices of 32 x 8: every diagonal length up to 30 (the serial launch has a
    thread for each slice of a diagonal), a multi-workgroup grid in the parallel launches"""
    P, planes, res = K.expected("large")
    assert_same(run(ctx, P, [planes])[0], res)


def test_diagonals_longer_than_the_serial_workgroup(ctx):
    """68 x 66 slices whose LL rectangles limit the serial launch to 64 threads (lowdelay_enc_cases.turns_case): diagonals of
    up to 66 slices, so a thread takes slices in turns, and the ones of the second turn need the whole search"""
    P, planes, res = K.expected("turns")
    assert min(P["n_horiz_slices"], P["n_vert_slices"]) > 64 and res["index"].reshape(66, 68)[64:].min() > 0
    assert_same(run(ctx, P, [planes])[0], res)


@pytest.mark.parametrize("name", [n for n, c in K.CASES.items() if c[3] is None] + ["large"])
def test_round_trip_on_the_device(ctx, name):
    """schro_hip_lowdelay_batch of the produced bytes is the checker's reconstruction, on the input classes where the
    CPU test (test_lowdelay_enc_ref.py) found that a decoder can return it"""
    P, planes, res = K.expected(name)
    (data, _, count), = ctx.lowdelay_encode_batch([[ctx.upload(p) for p in planes]], P)
    assert count == 0 and np.array_equal(data, res["bytes"])
    out = [ctx.plane(p.shape[0], p.shape[1], np.int16) for p in planes]
    ctx.lowdelay_batch([(ctx.upload_bytes(data), out)], P)
    for k in range(3):
        assert np.array_equal(out[k].download(), res["recon"][k]), "component %d" % k


@pytest.mark.parametrize("name", ["64x32_d3_420", "72x40_5x3"])
def test_frame_layer_is_the_plane_layer(ctx, name):
    P, planes, res = K.expected(name)
    fmt = {(1, 1): 420, (1, 0): 422, (0, 0): 444}
    hs = int(P["iwt_chroma_width"] < P["iwt_luma_width"])
    vs = int(P["iwt_chroma_height"] < P["iwt_luma_height"])
    assert (hs, vs) in fmt
    # a frame whose components hold the iwt sizes (72 x 40 4:2:2: the chroma iwt width, 40, is more than half of 72)
    width = max(P["iwt_luma_width"], P["iwt_chroma_width"] << hs)
    height = max(P["iwt_luma_height"], P["iwt_chroma_height"] << vs)
    f = frames.DeviceFrame(ctx, frames.frame_format(np.int16, hs, vs), width, height)
    try:
        host = [np.zeros((f.c.components[k].height, f.c.components[k].width), np.int16) for k in range(3)]
        for h, p in zip(host, planes):
            h[:p.shape[0], :p.shape[1]] = p
        f.upload(frames.HostFrame(host, hs, vs))
        data, index, count = ctx.encode_lowdelay(f, P)
        assert_same((data, index, count), res)
        after = f.download()
        assert all(np.array_equal(a, h) for a, h in zip(after, host))       # the frame is not written
    finally:
        f.unref()


def test_refusals(ctx):
    """s32, the chroma LL mismatch, a wrong buffer size, bad strides, a non-positive denominator, LL bands or LL
    rectangles beyond what the kernels index: SCHRO_HIP_EINVAL with the
    member named, and nothing launched -- the guarded buffers keep their canaries"""
    P, planes, _ = K.expected(K.REFUSED_CASE)
    lay = G.Layout()
    comp = [lay.plane(p.shape[0], p.shape[1], np.int16, footprint=None) for p in planes]
    nbytes = P["slice_bytes_num"] * 16 // P["slice_bytes_denom"]
    sl, ix, cn = lay.span(nbytes), lay.span(16), lay.span(4)
    blk = G.GuardedBlock(ctx, lay, seed=5)

    class Shaped:
        def __init__(self, plane, **kw):
            self.ptr, self.stride, self.width, self.dtype = plane.ptr, plane.stride, plane.width, plane.dtype
            self.__dict__.update(kw)

    try:
        good = [blk[c] for c in comp]

        def refused(word, P=P, planes=good, slices=blk[sl], bpp=None):
            with pytest.raises(sa.SchroHipError) as e:
                ctx.lowdelay_encode_batch([(planes, slices, blk[ix], blk[cn])], P, bpp=bpp)
            assert word in str(e.value), str(e.value)

        refused("s32", bpp=4)
        refused("slices_bytes", slices=Shaped(blk[sl], width=nbytes - 1))
        refused("stride[1]", planes=[good[0], Shaped(good[1], stride=good[1].stride - 2), good[2]])
        refused("stride[0]", planes=[Shaped(good[0], stride=good[0].stride + 1), good[1], good[2]])
        refused("comp[2]", planes=[good[0], good[1], Shaped(good[2], ptr=good[2].ptr + 1)])
        # the parameters: the chroma LL mismatch, the denominators, and what the kernels index with int
        changed = K.refused_params(P)
        assert [w for w, _ in changed] == ["chroma LL", "slice_bytes_denom", "slice_bytes_denom", "LL bands", "LL rectangles"]
        for word, bad in changed:
            refused(word, P=bad)
        ctx.synchronize()
        blk.check()
    finally:
        blk.free()
